#!/usr/bin/env python3
"""Generates tests/golden/forgeries.json from the CPU oracle: groups of signature sets whose errors
cancel under an unblinded (or affinely weighted) sum, and the sets of the edge-word test.

A forged signature is sk H(m) + k D with D = 7 H("cancel-offset") in G2: the set alone is invalid, but
a group whose k sum to zero passes the batch equation with equal scalars, and the triple (1, -2, 1)
passes it with ANY affine scalar sequence a + b i (sum k_i = sum i k_i = 0), such as the weights
c + 1 of the invalid-set search's weighted tests.  Only independent per-set blinding words reject
them.  Each group is a list of {pubkeys: [96-byte hex ...], signing_root, signature}:

  pair_same_root      two 1-key sets over one root, offsets +D, -D
  triple_same_root    three 1-key sets over one root, offsets +D, -2D, +D
  pair_aggregate      as pair_same_root, each set over two pubkeys
  pair_sibling_roots  two 1-key sets over two roots (not those of cancel_pair.json), +D, -D
  negated_valid_pair  two VALID sets over one root, (PK, m, sig) and (-PK, m, -sig): under one
                      shared blinding word the root's sum r PK is the point at infinity
  edge_words          six valid sets, each on a root of its own, and one wrong-message set (last)

Run from the repo root:
    python3 tests/golden/make_forgeries.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls_oracle as o  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def root(tag):
    return bytes([tag]) * 32


def entry(pks, m, sig):
    return {"pubkeys": [o.g1_serialize(pk).hex() for pk in pks], "signing_root": m.hex(),
            "signature": o.g2_compress(sig).hex()}


def forged(d, keys, m, k):
    """one set over the interop keys `keys`, signed over m, offset by k D"""
    sks = [o.interop_secret_key(i) for i in keys]
    sig = o.g2_mul(o.hash_to_g2(m), sum(sks) % o.R)
    if k:
        sig = o.g2_add(sig, o.g2_mul(d, k % o.R))
    return entry([o.sk_to_pk(sk) for sk in sks], m, sig)


def main():
    d = o.g2_mul(o.hash_to_g2(b"cancel-offset"), 7)
    groups = {
        "pair_same_root": [forged(d, [5], root(0xC3), 1), forged(d, [6], root(0xC3), -1)],
        "triple_same_root": [forged(d, [7], root(0xD4), 1), forged(d, [8], root(0xD4), -2),
                             forged(d, [9], root(0xD4), 1)],
        "pair_aggregate": [forged(d, [10, 11], root(0xE5), 1), forged(d, [12, 13], root(0xE5), -1)],
        "pair_sibling_roots": [forged(d, [14], root(0xF6), 1), forged(d, [15], root(0x17), -1)],
    }
    sk, m = o.interop_secret_key(16), root(0x28)
    pk, sig = o.sk_to_pk(sk), o.sign(sk, m)
    groups["negated_valid_pair"] = [entry([pk], m, sig), entry([o.g1_neg(pk)], m, o.g2_neg(sig))]
    edge = [forged(d, [17 + i], root(0x31 + i), 0) for i in range(6)]
    wrong = forged(d, [23], root(0x3F), 0)       # signed over another root than the one it claims
    wrong["signing_root"] = root(0x37).hex()
    groups["edge_words"] = edge + [wrong]
    out = {"generator": "tests/golden/make_forgeries.py",
           "note": "forged sets: each alone verifies false, the group passes with equal scalars "
                   "(the triple with any affine sequence); negated_valid_pair and the first six of "
                   "edge_words are valid, the last of edge_words is signed over another root",
           "groups": groups}
    with open(os.path.join(OUT, "forgeries.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
