"""The drop-in pool's default minPackageSets ("Multi-GPU inside the drop-in").

Measures, on one GPU, sets/s of a lone package on one pool engine against package size: c3-shaped
packages (16 one-set attestation jobs to every 3-set aggregate job, 64 committees' roots) cut to
256, 512, ..., 16 384 sets, and one full slot (19 456 sets), each through the drop-in's path
(lb_verify_jobs_indexed: upload, verify, readback) on an engine created after the device's latency
engine, as the pool's engines are.  The default is the smallest power of two whose rate is at
least half the full slot's: two devices with s sets each then finish no later than one device
with 2 s sets at its best rate, so cutting a queue at that size cannot lose.

  python tools/min_package_sets.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lodestar_amd import workloads as W  # noqa: E402
from lodestar_amd.engine import Engine  # noqa: E402

SIZES = [256, 512, 1024, 2048, 4096, 8192, 16384]
FULL_SLOT = 16384 + 3 * 1024
REPS = 9


def c3_cut(engine, keys, n_sets):
    """c3's job mix at n_sets sets: one aggregate job (3 sets) to every 16 attestation jobs"""
    n_agg = round(n_sets / 19)
    return W.make(engine, "c3", keys=keys, n_att=n_sets - 3 * n_agg, n_agg=n_agg)


def main():
    latency = Engine(0, Engine.LATENCY)
    eng = Engine(0)
    keys = W.KeyPool(eng)
    curve = []
    for n in SIZES + [FULL_SLOT]:
        wl = c3_cut(eng, keys, n)
        assert wl.packed.n_sets == n
        packed = W.indexed_for(eng, wl)
        assert np.array_equal(np.asarray(eng.verify_jobs_packed(packed)), wl.expected)
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            eng.verify_jobs_packed(packed)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        med = ms[len(ms) // 2]
        curve.append({"sets": n, "jobs": wl.packed.n_jobs, "ms_median": round(med, 3), "ms_min": round(ms[0], 3),
                      "ms_max": round(ms[-1], 3), "sets_per_s": round(n / (med * 1e-3))})
        print(curve[-1], flush=True)
    full = curve[-1]["sets_per_s"]
    chosen = next(c["sets"] for c in curve[:-1] if c["sets_per_s"] >= full / 2)
    out = {"device_cus": eng.cu_count, "reps": REPS, "curve": curve, "full_slot_sets_per_s": full,
           "half_rate": full / 2, "min_package_sets": chosen}
    latency.close()
    eng.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
