#!/usr/bin/env python3
"""Host field against device field for the three ckzg calls, one process, one engine.

  python tools/kzg_field_ab.py [--calls 12] [--warmup 2] [--out profiles/kzg_device_field.json]

Per leg (blobToKzgCommitment of 1 blob, computeAggregateKzgProof and verifyAggregateKzgProof of
2 blobs) the two paths alternate call by call; medians, and each path's spread (min .. max) as its
run-to-run figure.  Two more timings name the stage that holds the device path: one 4096-term
lb_g1_lincomb (the MSM chain both paths share) and lb_kzg_blob_coefficients (upload, range
check, inverse NTT, download: the device field work of one blob).  Results are also checked for
equality, so a timing is never reported for differing bytes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lodestar_amd import kzg as K  # noqa: E402
from lodestar_amd.engine import Engine  # noqa: E402


def blob(off):
    b = bytearray(K.BYTES_PER_BLOB)
    for i in range(K.FIELD_ELEMENTS_PER_BLOB):
        b[32 * i: 32 * i + 4] = ((i + off) & 0xFFFFFFFF).to_bytes(4, "big")
    return bytes(b)


def ab(fa, fb, calls, warmup):
    ta, tb = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        ra = fa()
        t1 = time.perf_counter()
        rb = fb()
        t2 = time.perf_counter()
        assert ra == rb, "host and device paths disagree"
        if i >= warmup:
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
    return ta, tb


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "calls": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    blobs = [blob(0), blob(7)]
    with Engine(0) as e:
        host, dev = K.Kzg(e), K.Kzg(e, field="device")
        comms = [host.blobToKzgCommitment(b) for b in blobs]
        proof = host.computeAggregateKzgProof(blobs)
        legs = {
            "blobToKzgCommitment_1": (lambda: host.blobToKzgCommitment(blobs[0]), lambda: dev.blobToKzgCommitment(blobs[0])),
            "computeAggregateKzgProof_2": (lambda: host.computeAggregateKzgProof(blobs),
                                           lambda: dev.computeAggregateKzgProof(blobs)),
            "verifyAggregateKzgProof_2": (lambda: host.verifyAggregateKzgProof(blobs, comms, proof),
                                          lambda: dev.verifyAggregateKzgProof(blobs, comms, proof)),
        }
        res = {"legs": {}, "stages": {}}
        for name, (fh, fd) in legs.items():
            th, td = ab(fh, fd, a.calls, a.warmup)
            h, d = stats(th), stats(td)
            res["legs"][name] = {"host": h, "device": d, "host_over_device": round(h["median_ms"] / d["median_ms"], 2),
                                 # faster by more than the host's own spread?
                                 "device_faster_beyond_host_spread": h["median_ms"] - d["median_ms"] > h["max_ms"] - h["min_ms"]}
        coeffs = K.evaluations_to_coefficients(K.blob_to_polynomial(blobs[0]))
        t_msm, t_field = [], []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            c = host.g1_lincomb(coeffs)
            t1 = time.perf_counter()
            got = dev.blob_coefficients(blobs[0])
            t2 = time.perf_counter()
            assert c == comms[0] and got == coeffs
            if i >= a.warmup:
                t_msm.append((t1 - t0) * 1e3)
                t_field.append((t2 - t1) * 1e3)
        res["stages"]["g1_lincomb_4096 (MSM chain; includes packing 4096 Python ints)"] = stats(t_msm)
        res["stages"]["blob_coefficients (device field work of one blob; includes unpacking 4096 Python ints)"] = stats(t_field)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
