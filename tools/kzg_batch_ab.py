#!/usr/bin/env python3
"""A loop of single verifications against one batched verification, one process, one engine.

  python tools/kzg_batch_ab.py [--rounds 12] [--warmup 2] [--limit 120] [--out profiles/kzg_batch_ab.json]

For n = 1, 8 and 32 sidecars of two blobs each the two kinds alternate round by round:
  loop   n calls of lb_kzg_verify_aggregate_proof, one sidecar each
  batch  one call of lb_kzg_verify_aggregate_proof_batch over the n sidecars
Medians and each kind's spread (min .. max); `batch_max_below_loop_min` says whether the slowest
batch round beat the fastest loop round, which neither side's spread can produce.  The batch call's
host transcript hashing (lb_kzg_batch_hash_ns) is reported separately, with its share of the call.
Each kind runs under its own time limit: an alarm with the default disposition, which ends the
process even inside a native call.  The verdicts are checked, so a timing is never reported for a
wrong result."""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lodestar_amd import _native as N  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402
from lodestar_amd.engine import Engine  # noqa: E402

U8, U32, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)


def blob(off):
    b = bytearray(K.BYTES_PER_BLOB)
    for i in range(K.FIELD_ELEMENTS_PER_BLOB):
        b[32 * i: 32 * i + 4] = ((i + off) & 0xFFFFFFFF).to_bytes(4, "big")
    return bytes(b)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measured kind and round")
    ap.add_argument("--sizes", default="1,8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lib = N.load()
    res = {"blobs_per_sidecar": 2, "sizes": {}}
    with Engine(0) as e:
        dev = K.Kzg(e, field="device")
        # distinct sidecars: no two share a blob
        cars = []
        for k in range(max(sizes)):
            blobs = [blob(1000 * k), blob(1000 * k + 7)]
            comms = dev._device_commitments(blobs)
            cars.append((b"".join(blobs), b"".join(comms), dev.computeAggregateKzgProof(blobs)))
        for n in sizes:
            bl = np.frombuffer(b"".join(c[0] for c in cars[:n]), np.uint8)
            cm = np.frombuffer(b"".join(c[1] for c in cars[:n]), np.uint8)
            pf = np.frombuffer(b"".join(c[2] for c in cars[:n]), np.uint8)
            off = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
            singles = [(np.frombuffer(c[0], np.uint8), np.frombuffer(c[1], np.uint8), np.frombuffer(c[2], np.uint8))
                       for c in cars[:n]]

            def loop():
                ok = ctypes.c_int32(0)
                for sb, sc, sp in singles:
                    rc = lib.lb_kzg_verify_aggregate_proof(e.h, 2, sb.ctypes.data_as(U8), sc.ctypes.data_as(U8),
                                                           sp.ctypes.data_as(U8), ctypes.byref(ok))
                    assert rc == 0 and ok.value == 1, (rc, ok.value)

            def batch():
                out = np.zeros(n, np.int32)
                rc = lib.lb_kzg_verify_aggregate_proof_batch(e.h, n, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                             cm.ctypes.data_as(U8), pf.ctypes.data_as(U8),
                                                             out.ctypes.data_as(I32))
                assert rc == 0 and out.tolist() == [1] * n, (rc, out.tolist())

            t_loop, t_batch, t_hash = [], [], []
            for i in range(a.warmup + a.rounds):
                signal.alarm(a.limit)   # the loop's own limit
                t0 = time.perf_counter()
                loop()
                t1 = time.perf_counter()
                signal.alarm(a.limit)   # the batch call's own limit
                t2 = time.perf_counter()
                batch()
                t3 = time.perf_counter()
                signal.alarm(0)
                if i >= a.warmup:
                    t_loop.append((t1 - t0) * 1e3)
                    t_batch.append((t3 - t2) * 1e3)
                    t_hash.append(lib.lb_kzg_batch_hash_ns(e.h) / 1e6)
            lo, ba, ha = stats(t_loop), stats(t_batch), stats(t_hash)
            res["sizes"][str(n)] = {
                "loop_of_single_calls": lo, "batch_call": ba, "batch_host_hashing": ha,
                "loop_over_batch": round(lo["median_ms"] / ba["median_ms"], 2),
                "hashing_share_of_batch": round(ha["median_ms"] / ba["median_ms"], 3),
                "batch_max_below_loop_min": ba["max_ms"] < lo["min_ms"],
            }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
