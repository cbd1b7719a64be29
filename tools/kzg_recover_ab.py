#!/usr/bin/env python3
"""Cell recovery (lb_kzg_recover_cells_and_proofs) against lb_kzg_compute_cells_and_proofs (FK20 from the
blob's own bytes) on the same blob, one process, one engine, the FK20 table already built.

  python tools/kzg_recover_ab.py [--rounds 7] [--warmup 2] [--limit 120] [--out profiles/kzg_recover.json]

One blob recovered from cells 0 .. 63 alternates round by round with FK20 on that blob; medians and each
leg's spread (min .. max).  The gate: the recovery median is at most 1.10 x the FK20 median of the same
run -- what recovery adds to FK20 (the upload of 64 cells, 64 cell interpolations, 64 column decodes of
three 128-point scalar transforms, one more 4096-point transform) is small beside FK20's 8192 ladders,
and FK20's own spread in profiles/kzg_fk20.json is about +-4 %.  Then, ungated: six blobs recovered in
one call against one.  Each call runs under its own time limit: an alarm with the default disposition,
which ends the process even inside a native call.  The outputs of the two legs are compared before any
time is reported: recovery must give FK20's cells and proofs, byte for byte."""
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
HALF = CELLS // 2
GATE = 1.10


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measured call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = N.load()
    res = {"blobs": NB, "given_cells": "0..63", "gate": f"recover_1_blob median <= {GATE} x fk20_1_blob median"}

    def limited(fn):
        signal.alarm(a.limit)   # the call's own limit
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        signal.alarm(0)
        return (t1 - t0) * 1e3, out

    with Engine(0) as e:
        dev = K.Kzg(e, field="device")
        dev.load_trusted_setup(open(K.TRUSTED_SETUP_BIN, "rb").read())
        blobs = [blob(1000 * k) for k in range(NB)]
        bl = np.frombuffer(b"".join(blobs), np.uint8)
        # cells 0 .. 63 of a blob are the blob's own bytes
        off = (np.arange(NB + 1, dtype=np.uint32) * HALF).astype(np.uint32)
        idx = np.tile(np.arange(HALF, dtype=np.uint32), NB)

        def fk20(n):
            cells = np.zeros(n * CELLS * K.BYTES_PER_CELL, np.uint8)
            proofs = np.zeros(n * CELLS * 48, np.uint8)
            st = np.zeros(n, np.int32)
            rc = lib.lb_kzg_compute_cells_and_proofs(e.h, n, bl.ctypes.data_as(U8), cells.ctypes.data_as(U8),
                                                     proofs.ctypes.data_as(U8), st.ctypes.data_as(I32))
            assert rc == 0 and not st.any(), (rc, st.tolist())
            return cells.tobytes(), proofs.tobytes()

        def recover(n):
            cells = np.zeros(n * CELLS * K.BYTES_PER_CELL, np.uint8)
            proofs = np.zeros(n * CELLS * 48, np.uint8)
            st = np.zeros(n, np.int32)
            rc = lib.lb_kzg_recover_cells_and_proofs(e.h, n, off.ctypes.data_as(U32), idx.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                     cells.ctypes.data_as(U8), proofs.ctypes.data_as(U8), st.ctypes.data_as(I32))
            assert rc == 0 and not st.any(), (rc, st.tolist())
            return cells.tobytes(), proofs.tobytes()

        limited(lambda: fk20(1))                      # builds the table
        t = {"recover_1_blob": [], "fk20_1_blob": []}
        for i in range(a.warmup + a.rounds):
            ms_r, out_r = limited(lambda: recover(1))
            ms_f, out_f = limited(lambda: fk20(1))
            assert out_r == out_f, "recovery and FK20 disagree"
            if i >= a.warmup:
                t["recover_1_blob"].append(ms_r)
                t["fk20_1_blob"].append(ms_f)
        res["one_blob"] = {k: stats(v) for k, v in t.items()}
        r_med, f_med = res["one_blob"]["recover_1_blob"]["median_ms"], res["one_blob"]["fk20_1_blob"]["median_ms"]
        res["one_blob"]["recover_over_fk20"] = round(r_med / f_med, 3)
        res["one_blob"]["gate_met"] = bool(r_med <= GATE * f_med)

        want6 = fk20(NB)
        t6 = {"recover_6_blobs": [], "recover_1_blob": []}
        for i in range(a.warmup + a.rounds):
            ms6, out6 = limited(lambda: recover(NB))
            ms1, out1 = limited(lambda: recover(1))
            assert out6 == want6 and out1[0] == want6[0][: len(out1[0])] and out1[1] == want6[1][: len(out1[1])]
            if i >= a.warmup:
                t6["recover_6_blobs"].append(ms6)
                t6["recover_1_blob"].append(ms1)
        six = {k: stats(v) for k, v in t6.items()}
        six["six_over_one"] = round(six["recover_6_blobs"]["median_ms"] / six["recover_1_blob"]["median_ms"], 3)
        res["six_blobs"] = six
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["one_blob"]["gate_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
