"""tests/golden/edge_points.json through every GPU decode path: g2_decompress96_w in
k_decompress_sigs (aggregate_signatures, and verification with LB_ALONE=0), g2_decompress96_wp in
k_decompress_sigs_row (verification with LB_ALONE=1 LB_ROW_FE=1), g1_decompress48 in k_g1_decompress
and k_table_fill, g1_deserialize96 in k_table_fill and k_pk_chunks, with their validate branches.
The records are encodings an attacker can pick: x with x^3 + 4(1+i) in Fp or purely imaginary (the
Fp2 square root's delta = d2 and swapped-component branches, the sign decided by y.c0), fixed small
x, non-canonical and >= p coordinates, every flag combination, points of order 3 and 11 and a key
plus a point of order 3 for the [r]P == O key validation.  Every comparison is exact: byte strings
and status codes against the oracle's (tests/test_edge_points_cpu.py checks the fixture itself)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_json
from lodestar_amd.engine import SetInput
from test_gpu_parity import R, interop_sk
from test_subgroup28_gpu import _engine_with, _named

pytestmark = pytest.mark.gpu

G2_INF = bytes([0xC0]) + bytes(95)
EDGE_TAGS = {"y_c1_zero", "y_c0_zero", "rhs_c0_zero"}


def recs(kind):
    return [r for r in load_json("edge_points.json")["records"] if r["kind"] == kind]


def names(status):
    from lodestar_amd import _native as N
    return [N.error_name(s) for s in status]


def blst(status_name):
    """a fixture status as the name the library gives its code"""
    return "BLST_SUCCESS" if status_name in ("ok", "inf") else status_name


@pytest.fixture(scope="module")
def valid_sets(engine):
    """64 valid one-key sets signed on the GPU, for padding and interleaving"""
    rng = np.random.default_rng(96)
    pool = [interop_sk(i) for i in range(16)]
    _, pk96 = engine.sk_to_pk(pool)
    msgs = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    idx = rng.integers(0, 16, size=64)
    sigs = engine.sign([pool[j] % R for j in idx], msgs)
    return [SetInput([pk96[idx[i]].tobytes()], msgs[i].tobytes(), sigs[i].tobytes()) for i in range(64)]


# ---------------------------------------------------------------------------- G2: aggregate_signatures
def test_g2_round_trip_through_aggregate_signatures(engine, valid_sets):
    """one group per record, padded with valid signatures to 65 groups (k_decompress_sigs: a full
    wave and a one-lane tail): unvalidated, the output is the input for every decodable record,
    the only public observation of the y-sign choice where y.c1 == 0"""
    g2 = recs("g2c96")
    sigs = [bytes.fromhex(r["hex"]) for r in g2]
    pad = [s.signature for s in valid_sets[:65 - len(sigs)]]
    assert len(sigs + pad) == 65 and len(pad) >= 1
    out, st = engine.aggregate_signatures([[b] for b in sigs + pad], validate=False)
    assert names(st) == [blst(r["status"]) for r in g2] + ["BLST_SUCCESS"] * len(pad)
    for r, b, got in zip(g2, sigs, out):
        if r["status"] == "ok":
            assert got == b, r["name"]
        elif r["status"] == "inf":
            assert got == G2_INF, r["name"]
    assert out[len(sigs):] == pad
    out, st = engine.aggregate_signatures([[b] for b in sigs + pad], validate=True)
    assert names(st) == [blst(r["status_validated"]) for r in g2] + ["BLST_SUCCESS"] * len(pad)
    assert out[len(sigs):] == pad


def test_g2_sums_of_edge_points(engine):
    """b + b, b - b, b + c and b + inf + c over the points with a zero y or rhs component"""
    import oracle.bls_oracle as o
    edge = [bytes.fromhex(r["hex"]) for r in recs("g2c96") if EDGE_TAGS & set(r["tags"])]
    assert len(edge) == 12
    neg = lambda b: bytes([b[0] ^ 0x20]) + b[1:]  # noqa: E731
    groups, cancelling = [], []
    for i, b in enumerate(edge):
        c = edge[(i + 5) % len(edge)]
        assert o.g2_decompress(neg(b)) == o.g2_neg(o.g2_decompress(b))
        cancelling.append(len(groups) + 1)
        groups += [[b, b], [b, neg(b)], [b, c], [b, G2_INF, c]]
    exp = []
    for g in groups:
        acc = None
        for b in g:
            acc = o.g2_add(acc, o.g2_decompress(b))
        exp.append(o.g2_compress(acc))
    assert all(exp[i] == G2_INF for i in cancelling)
    out, st = engine.aggregate_signatures(groups, validate=False)
    # a cancelling group is BLST_SUCCESS with 0xc0..., as aggregates.json defines it for [sig, -sig]
    assert names(st) == ["BLST_SUCCESS"] * len(groups)
    assert out == exp


# ---------------------------------------------------------------------------- G2: both decode kernels inside verify
@pytest.fixture(scope="module")
def decode_forms():
    """k_decompress_sigs for every batch (LB_ALONE=0), and k_decompress_sigs_row for batches up to
    dec_row_max = 4096 sets (the row engine: LB_ALONE=1 LB_ROW_FE=1)"""
    lane = _engine_with({"LB_ALONE": "0"})
    row = _engine_with({"LB_ALONE": "1", "LB_ROW_FE": "1"})
    yield {"lane": lane, "row": row}
    lane.close()
    row.close()


def _record_sets():
    fx = load_json("edge_points.json")
    key, root = bytes.fromhex(fx["key"]["pubkey96"]), bytes.fromhex(fx["key"]["signing_root"])
    g2 = [r for r in fx["records"] if r["kind"] == "g2c96"]
    return g2, [SetInput([key], root, bytes.fromhex(r["hex"])) for r in g2]


def test_every_g2_record_through_both_decode_kernels(decode_forms, valid_sets):
    """One-set jobs: each record's signature beside the fixture's key and root, so a job is what
    oracle.verify_job gave the generator (true only for the key's own signature; false, not an
    error, for its negation and for a valid signature of another key), interleaved with valid
    sets; the odd count leaves the last wave of k_decompress_sigs_row half full.  Neither
    last_profile() (one 'decode' stage for both kernels) nor the search trace names the decode
    kernel: the pinned LB_ALONE / LB_ROW_FE and n <= dec_row_max are the evidence for which ran."""
    g2, rsets = _record_sets()
    sets, exp = [valid_sets[0]], [True]
    for k, (r, s) in enumerate(zip(g2, rsets)):
        sets += [s, valid_sets[k + 1]]
        exp += [r["verify"], True]
    n = len(sets)
    assert n % 2 == 1 and n <= 4096 and n > 64
    assert "LB_DEC_ROW_MAX" not in os.environ
    jobs = [[s] for s in sets]
    lane = _named(decode_forms["lane"].verify_jobs(jobs))
    row = _named(decode_forms["row"].verify_jobs(jobs))
    assert lane == row
    assert lane == exp


def test_one_set_batches_of_each_tag(decode_forms):
    """n = 1 (one half-full wave of the row form) for the first record of every tag"""
    g2, rsets = _record_sets()
    first = {}
    for r, s in zip(g2, rsets):
        for t in r["tags"]:
            first.setdefault(t, (r, s))
    assert {"y_c1_zero", "y_c0_zero", "d1_zero", "rhs_c0_zero", "fixed_x", "bad_encoding", "flags", "infinity",
            "valid", "negated"} <= set(first)
    for t, (r, s) in sorted(first.items()):
        for form in ("row", "lane"):
            assert _named(decode_forms[form].verify_jobs([[s]])) == [r["verify"]], (t, r["name"], form)


# ---------------------------------------------------------------------------- G1
def test_g1_decompress_with_and_without_validation(engine):
    """k_g1_decompress over the 48-byte records padded to 65 keys; with validation the points of
    order 3 and 11 and key + order-3 are BLST_POINT_NOT_IN_GROUP, the infinity key BLST_PK_IS_INFINITY"""
    g1 = recs("g1c48")
    good = load_json("aggregates.json")["g1_decompress"]
    pad = [good[i % len(good)] for i in range(65 - len(g1))]
    keys = [bytes.fromhex(r["hex"]) for r in g1] + [bytes.fromhex(x["in48"]) for x in pad]
    assert len(keys) == 65
    for validate, field in ((False, "status"), (True, "status_validated")):
        out, st = engine.g1_decompress(keys, validate=validate)
        assert names(st) == [blst(r[field]) for r in g1] + ["BLST_SUCCESS"] * len(pad), field
        for r, got in zip(g1, out):
            if r[field] == "ok":
                assert got.hex() == r["point"], r["name"]
        assert [b.hex() for b in out[len(g1):]] == [x["out96"] for x in pad]
    by_tag = {t: r for r in g1 for t in r["tags"]}
    assert [by_tag[t]["status_validated"] for t in ("order3", "order11", "mixed", "infinity")] == \
        ["BLST_POINT_NOT_IN_GROUP"] * 3 + ["BLST_PK_IS_INFINITY"]


@pytest.mark.parametrize("kind", ["g1c48", "g1u96"])
@pytest.mark.parametrize("validate", [False, True])
def test_pubkey_table_append_and_indexed_verify(engine, kind, validate):
    """k_table_fill's statuses, then one indexed one-set job per appended row over the key's own
    signature: true through a row holding the key, false through the row holding its negation, the
    append's error through a rejected row, BLST_PK_IS_INFINITY through an unvalidated infinity row.
    A point outside G1 appended unvalidated keeps status 0 (the reference's unvalidated path); only
    its append status is asserted."""
    from lodestar_amd import _native as N
    fx = load_json("edge_points.json")
    g1 = [r for r in fx["records"] if r["kind"] == kind]
    field = "status_validated" if validate else "status"
    first, st = engine.pubkey_table_append([bytes.fromhex(r["hex"]) for r in g1], validate=validate)
    assert names(st) == [blst(r[field]) for r in g1]
    own = SetInput([], bytes.fromhex(fx["key"]["signing_root"]), bytes.fromhex(fx["key"]["signature"]))
    codes = engine.verify_jobs_indexed([[own]] * len(g1), [[[first + i]] for i in range(len(g1))])
    asserted = set()
    for r, s, code in zip(g1, st, codes):
        if s != 0:
            want = -s
        elif "key" in r["tags"]:
            want = 1
        elif "neg_key" in r["tags"]:
            want = 0
        elif "infinity" in r["tags"]:
            want = -N.LB_PK_IS_INFINITY
        else:
            assert "outside_g1" in r["tags"] and not validate, r["name"]
            continue
        assert code == want, r["name"]
        asserted.add(want)
    assert {1, 0, -N.LB_BAD_ENCODING, -N.LB_POINT_NOT_ON_CURVE, -N.LB_PK_IS_INFINITY} <= asserted
    assert (-N.LB_POINT_NOT_IN_GROUP in asserted) == validate


def test_aggregate_pubkeys_over_uncompressed_records(engine):
    """k_pk_chunks: every 96-byte record alone, and (0,2) + (0,2), (0,2) + (0,p-2), key + (0,2);
    expectations by the function that computes aggregates.json"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_golden import aggregate_pubkeys_case
    finally:
        sys.path.pop(0)
    g1 = recs("g1u96")
    by_name = {r["name"]: bytes.fromhex(r["hex"]) for r in g1}
    t3, t3n, key = by_name["order3"], by_name["order3_negated"], by_name["key"]
    assert t3 == bytes(47) + b"\x00" + bytes(47) + b"\x02" and t3n[:48] == t3[:48]
    groups = [[bytes.fromhex(r["hex"])] for r in g1] + [[t3, t3], [t3, t3n], [key, t3]]
    exp = [aggregate_pubkeys_case(g) for g in groups]
    assert exp[-3]["expected96"] == t3n.hex() and exp[-2]["expected96"] == (bytes([0x40]) + bytes(95)).hex()
    out, st = engine.aggregate_pubkeys(groups)
    assert names(st) == [e["status"] for e in exp]
    for e, got, s in zip(exp, out, st):
        if s == 0:
            assert got.hex() == e["expected96"]
