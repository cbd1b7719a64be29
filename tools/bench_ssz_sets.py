#!/usr/bin/env python3
"""Signing-root production from SSZ bytes (lb_block_sets_from_ssz) against the JSON walk, on the GPU.

  python tools/bench_ssz_sets.py [--reps 20] [--out profiles/ssz_sets_segment32.json] [--only-new]

Segment: 32 capella blocks of 128 attestations each with payloads of about 100 KB of transactions, through
the new call (signing_roots.block_signature_sets_ssz: bytes in, sets out) and, in the same run and
alternating with it, through the JSON route (block_signature_sets + resolve(GpuMerkleizer)).  Single block:
one such block through the new call, the JSON route with GpuMerkleizer and the JSON route with a hashlib
merkleizer.  Both routes start from what a node would hold for them (bytes / the parsed JSON object) and end
with every set's signing root as bytes and its keys looked up; times are host clocks around calls that end
in a stream synchronisation, medians over --reps after a warm-up.  The roots of the two routes are compared
before anything is timed.  --only-new runs the new call alone (for a kernel trace: rocprofv3 --kernel-trace
--stats -- python tools/bench_ssz_sets.py --only-new).
"""
import argparse
import copy
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ZH = [bytes(32)]
for _ in range(64):
    ZH.append(hashlib.sha256(ZH[-1] + ZH[-1]).digest())


def cpu_merkleize(trees):
    from lodestar_amd import signing_roots as SR
    out = []
    for t in trees:
        layer = SR.leaves(t)
        for d in range(t.depth):
            if len(layer) % 2:
                layer.append(ZH[d])
            layer = [hashlib.sha256(layer[i] + layer[i + 1]).digest() for i in range(0, len(layer), 2)]
        r = layer[0] if layer else ZH[t.depth]
        if t.mix is not None:
            r = hashlib.sha256(r + t.mix.to_bytes(32, "little")).digest()
        out.append(r)
    return out


def segment_blocks(k3, n_blocks=32, n_att=128, payload_bytes=100_000, n_tx=180):
    """n_blocks capella blocks (JSON) from the K3 devnet block: n_att attestations, n_tx transactions of
    payload_bytes in all (sizes from 100 B to a few KB, one of 20 KB), every block different"""
    import ssz_codec as C
    blocks = []
    for k in range(n_blocks):
        blk = copy.deepcopy(k3["signed_block"])
        m = blk["message"]
        m["slot"] = str(int(m["slot"]) + k)
        m["parent_root"] = "0x" + ("%02x" % k) * 32
        slot = int(m["slot"])
        m["body"]["attestations"] = [C.attestation(slot - 1 - i % 4, i % 64, 100 + (37 * i + k) % 400, "%02x" % ((i + k) & 255))
                                     for i in range(n_att)]
        sizes = [20_000] + [100 + (977 * i + 131 * k) % 900 for i in range(n_tx - 1)]
        scale = (payload_bytes - 20_000) / sum(sizes[1:])
        sizes = [sizes[0]] + [max(1, int(s * scale)) for s in sizes[1:]]
        m["body"]["execution_payload"]["transactions"] = [C.tx(s, (i + k) & 255) for i, s in enumerate(sizes)]
        blocks.append(blk)
    return blocks


def bench_state(k3):
    from lodestar_amd import signing_roots as SR
    committee = list(range(2048))
    return SR.StateView(genesis_validators_root=bytes.fromhex(k3["genesis_validators_root"]),
                        fork_previous_version=bytes.fromhex(k3["fork"]["previous_version"]),
                        fork_current_version=bytes.fromhex(k3["fork"]["current_version"]), fork_epoch=k3["fork"]["epoch"],
                        pubkey=lambda i: i, beacon_committee=lambda slot, index: committee,
                        sync_committee=lambda: committee[:512], fork_seq=lambda slot: SR.FORK_CAPELLA)


def median_ms(fns, reps):
    """medians (ms) of the callables, alternating them so that both see the same machine"""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)} for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-new", action="store_true")
    a = ap.parse_args()
    import ssz_codec as C
    from lodestar_amd import signing_roots as SR
    from lodestar_amd.engine import Engine
    with open(os.path.join(ROOT, "tests", "golden", "k3_devnet.json")) as f:
        k3 = json.load(f)
    blocks = segment_blocks(k3)
    raws = [C.encode_signed_block(b, 3) for b in blocks]
    st = bench_state(k3)
    states = [st] * len(blocks)
    with Engine(0) as e:
        def new_segment():
            return SR.block_signature_sets_ssz(e, raws, states)

        def json_segment():
            sets = [s for b in blocks for s in SR.block_signature_sets(b, st)]
            return SR.resolve(sets, SR.GpuMerkleizer(e))

        def new_single():
            return SR.block_signature_sets_ssz(e, raws[:1], states[:1])

        def json_single_gpu():
            return SR.resolve(SR.block_signature_sets(blocks[0], st), SR.GpuMerkleizer(e))

        def json_single_cpu():
            return SR.resolve(SR.block_signature_sets(blocks[0], st), cpu_merkleize)
        if a.only_new:
            for _ in range(a.reps):
                new_segment()
                new_single()
            print(json.dumps({"only_new": True, "reps": a.reps}))
            return
        got = [s for sets in new_segment() for s in sets]
        want = json_segment()
        assert [(s.name, s.signing_root, s.signature, s.pubkeys) for s in got] == \
            [(s.name, s.signing_root, s.signature, s.pubkeys) for s in want], "the two routes disagree"
        seg = median_ms([new_segment, json_segment], a.reps)
        one = median_ms([new_single, json_single_gpu, json_single_cpu], a.reps)
        # the call alone (no Python rows -> BlockSets), through the C ABI
        import ctypes
        import numpy as np
        P = lambda x, t: x.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
        n = len(raws)
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(r) for r in raws])
        ssz = np.frombuffer(b"".join(raws), dtype=np.uint8)
        dom = np.frombuffer(b"".join(SR.compute_domain(t, v, st.genesis_validators_root)
                                     for v in (st.fork_previous_version, st.fork_current_version)
                                     for t in SR._DOMAIN_ORDER) * n, dtype=np.uint8)
        forks, fe = np.full(n, 3, dtype=np.uint32), np.full(n, st.fork_epoch, dtype=np.uint64)
        ss = np.asarray([int(b["message"]["slot"]) for b in blocks], dtype=np.uint64)
        status, n_sets = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        kind, roots = np.zeros(199 * n, dtype=np.uint32), np.zeros(199 * n * 32, dtype=np.uint8)
        sigs, ref = np.zeros(199 * n * 96, dtype=np.uint8), np.zeros(199 * n * 4, dtype=np.uint64)

        def abi(nb):
            def f():
                rc = e.lib.lb_block_sets_from_ssz(e.h, nb, P(off, ctypes.c_uint32), P(ssz, ctypes.c_uint8),
                                                  P(forks, ctypes.c_uint32), P(dom, ctypes.c_uint8), P(fe, ctypes.c_uint64),
                                                  P(ss, ctypes.c_uint64), 0, P(status, ctypes.c_int32),
                                                  P(n_sets, ctypes.c_uint32), P(kind, ctypes.c_uint32), P(roots, ctypes.c_uint8),
                                                  P(sigs, ctypes.c_uint8), P(ref, ctypes.c_uint64))
                assert rc == 0
            return f
        call = median_ms([abi(n), abi(1)], a.reps)
    res = {
        "workload": {"blocks": len(blocks), "attestations_per_block": 128, "bytes_per_block": len(raws[0]),
                     "segment_bytes": sum(len(r) for r in raws), "sets": len(want), "reps": a.reps},
        "segment32": {"from_ssz": seg[0], "json_walk_gpu_merkleizer": seg[1], "lb_block_sets_from_ssz_call": call[0]},
        "single_block": {"from_ssz": one[0], "json_walk_gpu_merkleizer": one[1], "json_walk_cpu_merkleizer": one[2],
                         "lb_block_sets_from_ssz_call": call[1]},
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
