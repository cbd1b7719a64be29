#!/usr/bin/env python3
"""All 128 cell proofs of a blob by FK20 (lb_kzg_compute_cells_and_proofs) against the direct route
(lb_kzg_compute_cell_proofs over all 128 cells) on the same blob, one process, one engine.

  python tools/kzg_fk20_ab.py [--rounds 5] [--warmup 2] [--limit 120] [--out profiles/kzg_fk20.json]

The two legs alternate round by round, the table already built; medians and each leg's spread
(min .. max).  The gate: the FK20 median is at most one quarter of the direct route's.  Then, ungated:
six blobs in one call against one; six blobs against lb_kzg_blob_to_commitment on the same blobs (what
a producer pays anyway); and the one-off table build, as the first call after lb_kzg_load_setup minus
the steady call's median.  Each call runs under its own time limit: an alarm with the default
disposition, which ends the process even inside a native call.  The proofs of the two legs are
compared, so a timing is never reported for a wrong result."""
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
NB = 6
CELLS = K.CELLS_PER_EXT_BLOB


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measured call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = N.load()
    res = {"blobs": NB, "gate": "fk20_1_blob median <= direct_128_cells median / 4"}

    def limited(fn):
        signal.alarm(a.limit)   # the call's own limit
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        signal.alarm(0)
        return (t1 - t0) * 1e3, out

    with Engine(0) as e:
        dev = K.Kzg(e, field="device")
        blobs = [blob(1000 * k) for k in range(NB)]
        bl = np.frombuffer(b"".join(blobs), np.uint8)
        idx = np.arange(CELLS, dtype=np.uint32)

        def fk20(n):
            cells = np.zeros(n * CELLS * K.BYTES_PER_CELL, np.uint8)
            proofs = np.zeros(n * CELLS * 48, np.uint8)
            st = np.zeros(n, np.int32)
            rc = lib.lb_kzg_compute_cells_and_proofs(e.h, n, bl.ctypes.data_as(U8), cells.ctypes.data_as(U8),
                                                     proofs.ctypes.data_as(U8), st.ctypes.data_as(I32))
            assert rc == 0 and not st.any(), (rc, st.tolist())
            return proofs.tobytes()

        def direct():
            proofs = np.zeros(CELLS * 48, np.uint8)
            st = np.zeros(1, np.int32)
            rc = lib.lb_kzg_compute_cell_proofs(e.h, bl.ctypes.data_as(U8), CELLS, idx.ctypes.data_as(U32), proofs.ctypes.data_as(U8),
                                                st.ctypes.data_as(I32))
            assert rc == 0 and not st.any(), (rc, st.tolist())
            return proofs.tobytes()

        def commit(n):
            out = np.zeros(48 * n, np.uint8)
            st = np.zeros(n, np.int32)
            rc = lib.lb_kzg_blob_to_commitment(e.h, n, bl.ctypes.data_as(U8), out.ctypes.data_as(U8), st.ctypes.data_as(I32))
            assert rc == 0 and not st.any(), (rc, st.tolist())

        # the one-off table build: the first call after a setup load, three loads
        first = []
        for _ in range(3):
            dev.load_trusted_setup(open(K.TRUSTED_SETUP_BIN, "rb").read())
            first.append(limited(lambda: fk20(1))[0])

        t = {"fk20_1_blob": [], "direct_128_cells": []}
        for i in range(a.warmup + a.rounds):
            ms_f, pf = limited(lambda: fk20(1))
            ms_d, pd = limited(direct)
            assert pf == pd, "the two routes disagree"
            if i >= a.warmup:
                t["fk20_1_blob"].append(ms_f)
                t["direct_128_cells"].append(ms_d)
        res["one_blob"] = {k: stats(v) for k, v in t.items()}
        f_med, d_med = res["one_blob"]["fk20_1_blob"]["median_ms"], res["one_blob"]["direct_128_cells"]["median_ms"]
        res["one_blob"]["direct_over_fk20"] = round(d_med / f_med, 2)
        res["one_blob"]["gate_met"] = bool(f_med * 4 <= d_med)
        res["table_build"] = {"first_call_after_load": stats(first), "minus_steady_call_ms": round(statistics.median(first) - f_med, 3)}

        t6 = {"fk20_6_blobs": [], "fk20_1_blob": [], "blob_to_commitment_6_blobs": []}
        for i in range(a.warmup + a.rounds):
            ms6, p6 = limited(lambda: fk20(NB))
            ms1, p1 = limited(lambda: fk20(1))
            msc, _ = limited(lambda: commit(NB))
            assert p6[: len(p1)] == p1
            if i >= a.warmup:
                t6["fk20_6_blobs"].append(ms6)
                t6["fk20_1_blob"].append(ms1)
                t6["blob_to_commitment_6_blobs"].append(msc)
        six = {k: stats(v) for k, v in t6.items()}
        six["six_over_one"] = round(six["fk20_6_blobs"]["median_ms"] / six["fk20_1_blob"]["median_ms"], 3)
        six["six_over_commitments"] = round(six["fk20_6_blobs"]["median_ms"] / six["blob_to_commitment_6_blobs"]["median_ms"], 3)
        res["six_blobs"] = six
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["one_blob"]["gate_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
