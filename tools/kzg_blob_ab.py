#!/usr/bin/env python3
"""The per-blob batch verification against the aggregate-form batch verification on the same blobs,
one process, one engine.

  python tools/kzg_blob_ab.py [--rounds 12] [--warmup 2] [--limit 120] [--out profiles/kzg_blob_batch.json]

For each shape (groups x blobs per group: 1x1, 1x6, 32x2, 32x6) the two calls alternate round by round:
  aggregate  lb_kzg_verify_aggregate_proof_batch: one aggregate proof per group (the yardstick)
  blob       lb_kzg_verify_blob_proof_batch: one proof per blob, default hashing threads
and a third, `blob_1thread`, is the new call with LB_KZG_HASH_THREADS=1, for the hashing wall time
alone.  Medians and each kind's spread (min .. max); the host hashing time (lb_kzg_batch_hash_ns) is
reported per kind with its share of the call.  Each call runs under its own time limit: an alarm
with the default disposition, which ends the process even inside a native call.  The verdicts are
checked, so a timing is never reported for a wrong result."""
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
    ap.add_argument("--limit", type=int, default=120, help="seconds per measured call")
    ap.add_argument("--shapes", default="1x1,1x6,32x2,32x6")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    lib = N.load()
    threads = os.environ.get("LB_KZG_HASH_THREADS")
    res = {"hash_threads_default": int(threads) if threads else 8, "shapes": {}}
    with Engine(0) as e:
        dev = K.Kzg(e, field="device")
        total = max(g * b for g, b in shapes)
        blobs = [blob(1000 * k) for k in range(total)]   # distinct blobs
        comms = []
        for at in range(0, total, 32):
            comms += dev._device_commitments(blobs[at: at + 32])
        bl_all = np.frombuffer(b"".join(blobs), np.uint8)
        cm_all = np.frombuffer(b"".join(comms), np.uint8)
        proofs = np.zeros(48 * total, np.uint8)
        st = np.zeros(total, np.int32)
        signal.alarm(a.limit)
        rc = lib.lb_kzg_compute_blob_proofs(e.h, total, bl_all.ctypes.data_as(U8), cm_all.ctypes.data_as(U8),
                                            proofs.ctypes.data_as(U8), st.ctypes.data_as(I32))
        signal.alarm(0)
        assert rc == 0 and not st.any(), (rc, st.tolist())
        for g, b in shapes:
            nb = g * b
            bl, cm, pf = bl_all[: nb * K.BYTES_PER_BLOB], cm_all[: nb * 48], proofs[: nb * 48]
            off = np.arange(0, nb + 1, b, dtype=np.uint32)
            agg = np.frombuffer(b"".join(dev.computeAggregateKzgProof(blobs[k * b: (k + 1) * b]) for k in range(g)), np.uint8)

            def aggregate():
                out = np.zeros(g, np.int32)
                rc = lib.lb_kzg_verify_aggregate_proof_batch(e.h, g, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                             cm.ctypes.data_as(U8), agg.ctypes.data_as(U8),
                                                             out.ctypes.data_as(I32))
                assert rc == 0 and out.tolist() == [1] * g, (rc, out.tolist())

            def per_blob():
                out = np.zeros(g, np.int32)
                rc = lib.lb_kzg_verify_blob_proof_batch(e.h, g, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                        cm.ctypes.data_as(U8), pf.ctypes.data_as(U8), out.ctypes.data_as(I32))
                assert rc == 0 and out.tolist() == [1] * g, (rc, out.tolist())

            def timed(fn):
                signal.alarm(a.limit)   # the call's own limit
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                signal.alarm(0)
                return (t1 - t0) * 1e3, lib.lb_kzg_batch_hash_ns(e.h) / 1e6

            t = {"aggregate": [], "blob": [], "blob_1thread": []}
            h = {"aggregate": [], "blob": [], "blob_1thread": []}
            for i in range(a.warmup + a.rounds):
                for kind, fn in (("aggregate", aggregate), ("blob", per_blob), ("blob_1thread", per_blob)):
                    if kind == "blob_1thread":
                        os.environ["LB_KZG_HASH_THREADS"] = "1"
                    ms, hash_ms = timed(fn)
                    if kind == "blob_1thread":
                        if threads is None:
                            del os.environ["LB_KZG_HASH_THREADS"]
                        else:
                            os.environ["LB_KZG_HASH_THREADS"] = threads
                    if i >= a.warmup:
                        t[kind].append(ms)
                        h[kind].append(hash_ms)
            entry = {}
            for kind in t:
                ts, hs = stats(t[kind]), stats(h[kind])
                entry[kind] = {"call": ts, "host_hashing": hs, "hashing_share": round(hs["median_ms"] / ts["median_ms"], 3)}
            entry["blob_over_aggregate"] = round(entry["blob"]["call"]["median_ms"] / entry["aggregate"]["call"]["median_ms"], 3)
            res["shapes"][f"{g}x{b}"] = entry
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
