#!/usr/bin/env python3
"""The cell batch verification (EIP-7594) against the per-blob batch verification on the same six
blobs, one process, one engine.

  python tools/kzg_cells_ab.py [--rounds 12] [--warmup 2] [--limit 120] [--out profiles/kzg_cells_batch.json]

The yardstick is lb_kzg_verify_blob_proof_batch on 1 group x 6 blobs (the Deneb call a block's
sidecars go through).  It alternates round by round with lb_kzg_verify_cell_proof_batch on the same
blobs' cells:
  cells_768_1group     all 128 columns x 6 blobs in one group
  cells_768_128groups  128 groups of 6: one group per column (a node that holds every column)
  cells_48_1group      8 columns x 6 blobs in one group
  cells_48_8groups     the same as 8 groups of 6 (a node that samples 8 columns)
Medians and each kind's spread (min .. max); the host hashing time (lb_kzg_batch_hash_ns) is reported
per kind with its share of the call.  Then compute_cells beside blob_to_commitment, ms per blob at 1
and 6 blobs.  The cell proofs come from lb_kzg_compute_cell_proofs (one multi-scalar multiplication
per cell: the slow part of the set-up).  Each call runs under its own time limit: an alarm with the
default disposition, which ends the process even inside a native call.  The verdicts are checked, so a
timing is never reported for a wrong result."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = N.load()
    threads = os.environ.get("LB_KZG_HASH_THREADS")
    res = {"hash_threads_default": int(threads) if threads else 8, "blobs": NB}

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
        comms = dev._device_commitments(blobs)
        bl = np.frombuffer(b"".join(blobs), np.uint8)
        cm = np.frombuffer(b"".join(comms), np.uint8)
        proofs = np.zeros(48 * NB, np.uint8)
        st = np.zeros(NB, np.int32)
        _, rc = limited(lambda: lib.lb_kzg_compute_blob_proofs(e.h, NB, bl.ctypes.data_as(U8), cm.ctypes.data_as(U8),
                                                               proofs.ctypes.data_as(U8), st.ctypes.data_as(I32)))
        assert rc == 0 and not st.any(), (rc, st.tolist())
        # the cells and their proofs, per blob
        cells, cproofs = [], []
        setup_ms = 0.0
        for b in blobs:
            ms, c = limited(lambda: dev.compute_cells(b))
            cells.append(c)
            ms, p = limited(lambda: dev.compute_cell_kzg_proofs(b, list(range(K.CELLS_PER_EXT_BLOB))))
            setup_ms += ms
            cproofs.append(p)
        res["cell_proof_setup_ms_per_cell"] = round(setup_ms / (NB * K.CELLS_PER_EXT_BLOB), 3)

        def cell_call(columns, per_group):
            """column-major cells of the chosen columns in groups of per_group cells"""
            pos = [(b, j) for j in columns for b in range(NB)]
            n_cells = len(pos)
            c48 = np.frombuffer(b"".join(comms[b] for b, _ in pos), np.uint8)
            idx = np.asarray([j for _, j in pos], np.uint32)
            ce = np.frombuffer(b"".join(cells[b][j] for b, j in pos), np.uint8)
            pf = np.frombuffer(b"".join(cproofs[b][j] for b, j in pos), np.uint8)
            off = np.arange(0, n_cells + 1, per_group, dtype=np.uint32)
            g = len(off) - 1

            def call():
                out = np.zeros(g, np.int32)
                rc = lib.lb_kzg_verify_cell_proof_batch(e.h, g, off.ctypes.data_as(U32), c48.ctypes.data_as(U8),
                                                        idx.ctypes.data_as(U32), ce.ctypes.data_as(U8), pf.ctypes.data_as(U8),
                                                        out.ctypes.data_as(I32))
                assert rc == 0 and out.tolist() == [1] * g, (rc, out.tolist())
            return call

        off6 = np.asarray([0, NB], np.uint32)

        def yardstick():
            out = np.zeros(1, np.int32)
            rc = lib.lb_kzg_verify_blob_proof_batch(e.h, 1, off6.ctypes.data_as(U32), bl.ctypes.data_as(U8), cm.ctypes.data_as(U8),
                                                    proofs.ctypes.data_as(U8), out.ctypes.data_as(I32))
            assert rc == 0 and out.tolist() == [1], (rc, out.tolist())

        sampled = [0, 17, 34, 51, 64, 85, 102, 127]
        kinds = [("blob_1x6", yardstick),
                 ("cells_768_1group", cell_call(range(128), 768)),
                 ("cells_768_128groups", cell_call(range(128), NB)),
                 ("cells_48_1group", cell_call(sampled, 48)),
                 ("cells_48_8groups", cell_call(sampled, NB))]
        t = {k: [] for k, _ in kinds}
        h = {k: [] for k, _ in kinds}
        for i in range(a.warmup + a.rounds):
            for kind, fn in kinds:
                ms, _ = limited(fn)
                if i >= a.warmup:
                    t[kind].append(ms)
                    h[kind].append(lib.lb_kzg_batch_hash_ns(e.h) / 1e6)
        verify = {}
        for kind in t:
            ts, hs = stats(t[kind]), stats(h[kind])
            verify[kind] = {"call": ts, "host_hashing": hs, "hashing_share": round(hs["median_ms"] / ts["median_ms"], 3)}
        for kind in t:
            if kind != "blob_1x6":
                verify[kind]["over_blob_1x6"] = round(verify[kind]["call"]["median_ms"] / verify["blob_1x6"]["call"]["median_ms"], 3)
        res["verify"] = verify

        # compute_cells beside blob_to_commitment on the same blobs
        def c_cells(n):
            out = np.zeros(n * K.CELLS_PER_EXT_BLOB * K.BYTES_PER_CELL, np.uint8)
            s = np.zeros(n, np.int32)
            rc = lib.lb_kzg_compute_cells(e.h, n, bl.ctypes.data_as(U8), out.ctypes.data_as(U8), s.ctypes.data_as(I32))
            assert rc == 0 and not s.any()
            assert out[: K.BYTES_PER_BLOB].tobytes() == blobs[0]

        def c_commit(n):
            out = np.zeros(48 * n, np.uint8)
            s = np.zeros(n, np.int32)
            rc = lib.lb_kzg_blob_to_commitment(e.h, n, bl.ctypes.data_as(U8), out.ctypes.data_as(U8), s.ctypes.data_as(I32))
            assert rc == 0 and out.tobytes() == cm[: 48 * n].tobytes()

        produce = {}
        for n in (1, NB):
            tc, tk = [], []
            for i in range(a.warmup + a.rounds):
                ms_c, _ = limited(lambda: c_cells(n))
                ms_k, _ = limited(lambda: c_commit(n))
                if i >= a.warmup:
                    tc.append(ms_c / n)
                    tk.append(ms_k / n)
            produce[f"{n}_blobs"] = {"compute_cells_ms_per_blob": stats(tc), "blob_to_commitment_ms_per_blob": stats(tk)}
        res["produce"] = produce
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
