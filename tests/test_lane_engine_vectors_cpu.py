"""The conditions under which tests/test_lane_engines_gpu.py means something, checked with the
models alone (tools/gen_row_programs.py, tools/gen_wave_programs.py): every class of
tests/lane_engine_vectors.py holds the records it is meant to hold, and on every record the
model's result meets the exact conditions the GPU test then asks of the device."""
import pytest

import lane_engine_vectors as V

R, G, P = V.R, V.G, V.P


@pytest.fixture(scope="module")
def recs():
    return V.all_records()


def _units(n, rest):
    d = {"unit_%d" % k: n for k in range(12)}
    d.update(rest)
    return d


_PRODUCT = {"edge_limbs_2p": 240, "edge_limbs_32p": 240, "edge_limbs_only": 40, "random_2p": 40, "range_end": 8,
            "zero_x": 9, "zero_y": 8, "canonical": 18, "m_one": 4, "m_all_ones": 4, "m_alternating": 8,
            "m_random": 96, "m_zero_pow2": 56, "columns_low_cancel": 36, "columns_top_only": 24, "low_half_exact": 15}
_R1_MUL = dict(_PRODUCT, edge_limbs_2p=80, edge_limbs_32p=80, edge_limbs_only=14, random_2p=13, low_half_exact=5)
_R1_SQR = {k: 2 * v for k, v in _R1_MUL.items()}
_RFP = {"edge_limbs_2p": 150, "near_multiple_of_p": 84, "canonical": 9, "range_end": 4}
_OPERAND = dict({"edge_limb_terms_n%d" % n: 25 for n in range(1, 9)}, kp_plus_d=275, limb_sums_at_bound=4)
_CANON = {"residue_0": 12, "residue_1": 16, "residue_p_minus_1": 16, "residue_random": 192, "residue_edgy": 192,
          "edge_limbs": 120, "range_end": 4}
_IMPORT = {"value_0": 1, "value_1": 1, "value_p_minus_1": 1, "value_top": 1, "value_random": 60, "value_edgy": 40,
           "near_multiple_of_p": 312}
_WLIN_P = {"kp_plus_d": 946, "next_to_kp_top_limbs_exact": 190, "nn_zero": 50, "np_zero": 50, "max_terms": 44, "one_term": 36, "special_values": 45,
           "limb_sums_at_bound": 15, "top_limbs_zero": 30, "random_terms": 200}
_WLIN_L = dict(_WLIN_P, kp_plus_d=968, next_to_kp_top_limbs_exact=484, top_limbs_zero=72)
_F12 = _units(1, {"zero": 1, "one": 1, "minus_one": 1, "all_p_minus_1": 1, "sparse_line": 2, "cyclotomic": 2, "random": 3})
_F12_MUL = {k: 3 * v for k, v in _F12.items()}
_F12_FROB = {"zero": 1, "one": 1, "all_p_minus_1": 1, "unit_3": 1, "unit_10": 1, "sparse_line": 2, "cyclotomic": 2, "random": 3}
_F12_ONE = dict(_F12, one_plus_last=1, p_minus_1_first=1)
_F12_INV = {k: v for k, v in _F12.items() if k != "zero"}
_F12_EQ = {k + s: v for k, v in _F12.items() for s in ("_same", "_one_off")}

COUNTS = {
    "rp_mul": _PRODUCT, "r1_mul": _R1_MUL, "r1_sqr": _R1_SQR,
    "r_reduce": {"kp_plus_d": 1365, "one_term": 86, "limb_sums_at_bound": 8, "top_limbs_zero": 40,
                 "edge_limb_terms": 300, "next_to_kp_top_limbs_exact": 1202, "lanes_14_15_set": 24, "max_terms": 40},
    "f_add": _RFP, "f_sub": _RFP, "f_neg": _RFP, "f_mul3": _RFP, "f_mul8": _RFP, "f_mul": _RFP,
    "r_operand_carry": _OPERAND, "r_operand_red": dict(_OPERAND, kp_plus_d=297, coefficient_12=10),
    "r_canon": _CANON, "r_export": _CANON, "r1_export": _CANON,
    "r_import_export": _IMPORT, "r1_import_export": _IMPORT,
    "w_lin_maxp": _WLIN_P, "w_lin_maxp_full": _WLIN_P, "w_lin_maxl": _WLIN_L, "w_lin_maxl_full": _WLIN_L,
    "g_reduce": _WLIN_L, "g_reduce_full": _WLIN_L,
    "r_mul": _F12_MUL, "w_mul": _F12_MUL, "r_sqr": _F12, "w_sqr": _F12, "w_conj": _F12,
    "r_frob": _F12_FROB, "r_frob2": _F12_FROB, "w_frob": _F12_FROB, "w_frob2": _F12_FROB,
    "r_is_one": _F12_ONE, "w_is_one": _F12_ONE, "r_csqr": {"one": 1, "cyclotomic": 2}, "r_eq": _F12_EQ,
    "w_inv": _F12_INV, "r_pdbl_fast": {"chain_1": 1, "chain_2": 1, "chain_%d" % V.PDBL_CHAIN: 1},
}


def test_every_class_holds_its_records(recs):
    """the per-class counts, so that a change to the generator cannot empty a class unnoticed"""
    got = V.class_counts(recs)
    assert sorted(got) == sorted(COUNTS) == sorted(V.OPS)
    for name in COUNTS:
        assert got[name] == COUNTS[name], name
        assert all(n >= 1 for n in got[name].values()) and sum(got[name].values()) <= V.MAX_RECORDS


def test_vectors_are_deterministic_and_pack(recs):
    again = {"rp_mul": V.rp_mul_records(), "w_lin_maxp": V.w_lin_records(V.MAXP), "r_canon": V.canon_records()}
    for name, rs in again.items():
        assert [r.words for r in rs] == [r.words for r in recs[name]], name
    data = V.pack_input(recs)
    assert len(data) == 8 + sum(16 + 4 * len(rs) * V.OPS[n][1] for n, rs in recs.items())
    out = V.parse_output(bytes(4 * sum(len(rs) * V.OPS[n][2] for n, rs in recs.items())), recs)
    assert all(len(out[n]) == len(recs[n]) for n in recs)


def _none_wrong(name, rec, err):
    assert err is None, "%s, class %s: %s" % (name, rec.cls, err)


def test_row_products_on_the_model(recs):
    """congruent to x y / 2^392, |r| < |x y| / 2^392 + 1.0001 p, limbs in the slot range; the
    constructed records have the Montgomery factor they were built for; the column classes have
    the columns they are named after"""
    lo, hi = 0, 0
    for name in ("rp_mul", "r1_mul", "r1_sqr", "f_mul"):
        for rec in recs[name]:
            r = R.rp_mul(rec.x, rec.y)
            _none_wrong(name, rec, V.exact_row_product(rec.x, rec.y, r))
            lo, hi = min(lo, min(r[:13])), max(hi, max(r[:13]))
    assert V.LIMB_LO <= lo and hi < V.LIMB_HI
    for rec in recs["rp_mul"]:
        if hasattr(rec, "m"):
            assert V.mont_m(rec.x, rec.y) == rec.m, rec.cls
        assert abs(R.val(rec.x)) < 32 * P and abs(R.val(rec.y)) < 32 * P, rec.cls
        if rec.cls == "columns_top_only":
            U = V._u_columns(rec.x, rec.y)
            assert not any(U[:11]) and all(abs(u) > 1 << 40 for u in U[11:14])
        if rec.cls == "columns_low_cancel":
            x, y = (rec.x, rec.y) if V.B28 in rec.x else (rec.y, rec.x)
            cols = [sum(x[i] * y[k - i] for i in range(k + 1)) for k in range(14)]
            assert R.val(x) == 0 and not any(cols[11:]) and sum(1 for c in cols[:11] if abs(c) > 1 << 40) >= 8
        if rec.cls == "low_half_exact":
            U = V._u_columns(rec.x, rec.y)
            assert not any(U[:13]) and U[13] != 0 and U[13] % V.B28 == 0
    signs = {(R.val(r.x) > 0, R.val(r.y) > 0) for r in recs["rp_mul"] if r.cls.startswith("edge_limbs")}
    assert len(signs) == 4


def test_row_sums_on_the_model(recs):
    """reduced sums: congruent and within [-p / 2^20, p + p / 2^20); carry-only sums: the value
    itself; limbs in the slot range.

    The limb range: the row engine's header gave [-1, 2^28 + 2) and test_row_programs.py asserted
    [-2, 2^28 + 3).  On all of these vectors the model's limbs 0..12 span exactly [-1, 2^28]: -1 and
    2^28 are both attained, 2^28 + 1 is not.  2^28 + 1 stays admitted because the second carry
    round can hand on a carry of 2 when a column's carry has a third 28-bit piece (products only:
    a column of ~2^60), which these vectors never meet; so the range asserted everywhere is the
    header's [-1, 2^28 + 2), and this test pins what was measured."""
    lo, hi = 0, 0

    def see(r):
        nonlocal lo, hi
        lo, hi = min(lo, min(r[:13])), max(hi, max(r[:13]))

    for rec in recs["r_reduce"]:
        r = R.lin([(1, rec.acc)])
        see(r)
        _none_wrong("r_reduce", rec, V.exact_row_sum(rec.v, r, True))
    for name, red in (("r_operand_carry", False), ("r_operand_red", True)):
        for rec in recs[name]:
            assert 1 <= len(rec.terms) <= 8 and (red or sum(abs(c) for c, _ in rec.terms) <= 16)
            r = R.lin(rec.terms, reduce=red)
            see(r)
            _none_wrong(name, rec, V.exact_row_sum(rec.v, r, red))
            assert abs(R.val(r)) < 32 * P
    for name in V.RFP_TERMS:
        for rec in recs[name]:
            t = V.rfp_terms(name, rec)
            r = R.lin(t)
            see(r)
            _none_wrong(name, rec, V.exact_row_sum(sum(c * R.val(l) for c, l in t), r, True))
    for rec in recs["r_import_export"]:
        assert rec.a < P
        r = R.lin([(1, R.limbs(rec.a << 8))])
        see(r)
        _none_wrong("r_import_export", rec, V.exact_row_sum(rec.a << 8, r, True))
    assert (lo, hi) == (-1, V.B28), (lo, hi - V.B28)
    assert sum(1 for r in recs["r_reduce"] if r.cls == "top_limbs_zero" and max(map(abs, r.acc)) > V.B28) >= 30
    # the quotient range: |c| <= 7 over 24 slot values in (-2p, 2p)
    ks = [rec.k for rec in recs["r_reduce"] if rec.cls == "kp_plus_d"]
    assert min(ks) == -300 and max(ks) == 300
    top = max(abs(rec.v) for rec in recs["r_reduce"] if len(rec.terms) == 24)
    assert top == 24 * 7 * (2 * P - 1)
    for rec in recs["r_reduce"]:
        if rec.cls == "next_to_kp_top_limbs_exact":
            assert not any(rec.acc[:12]) and abs(rec.d) <= 1 << 336 and rec.v == rec.k * P + rec.d
            continue
        assert all(abs(c) <= 7 and abs(R.val(l)) < 2 * P for c, l in rec.terms), rec.cls
        if rec.cls == "kp_plus_d":
            assert rec.v == rec.k * P + rec.d and rec.d in V.DS
        if rec.cls == "top_limbs_zero":
            assert rec.acc[12] == 0 and rec.acc[13] == 0


def test_canonical_records(recs):
    """the representatives lie in (-2p, 2p), every residue class in more than one of them and in
    more than one spelling, with limbs in the slot range"""
    by = {}
    for rec in recs["r_canon"]:
        assert abs(rec.v) < 2 * P and rec.v == R.val(rec.x)
        assert all(V.LIMB_LO <= x < V.LIMB_HI for x in rec.x[:13]), rec.cls
        by.setdefault((rec.cls, rec.v % P), []).append(rec)
    for (cls, a), rs in by.items():
        if cls.startswith("residue") and cls != "residue_random":  # (generic limbs have one spelling)
            assert len({r.v for r in rs}) >= 3 and len({tuple(r.x) for r in rs}) > len({r.v for r in rs}), cls
    assert any(-1 in r.x[:13] for r in recs["r_canon"]) and any(V.B28 + 1 in r.x[:13] for r in recs["r_canon"])


@pytest.mark.parametrize("name", ["w_lin_maxp", "w_lin_maxl", "g_reduce"])
def test_wave_sums_on_the_model(recs, name):
    """V - (q - 1) p lies in [0, 3p) and is congruent to V; the terms respect the engines' bounds
    (coefficients <= 7, values < 3p, at most MAXN terms) and span the quotient range"""
    maxn = V.MAXP if name == "w_lin_maxp" else V.MAXL
    for rec in recs[name]:
        assert len(rec.pa) + len(rec.na) <= maxn
        assert all(0 <= c <= 7 and 0 <= x < 3 * P for c, x in rec.pa + rec.na), rec.cls
        assert rec.v == sum(c * x for c, x in rec.pa) - sum(c * x for c, x in rec.na)
        for full in (False, True):
            r = V.model_wave_sum(rec, full)
            assert 0 <= r < 1 << 384, (name, rec.cls)
            _none_wrong(name, rec, V.exact_wave_sum(rec.v, V.fp_words(r), full))
        if rec.cls in ("kp_plus_d", "next_to_kp_top_limbs_exact"):
            assert rec.v == rec.k * P + rec.d
        if rec.cls == "next_to_kp_top_limbs_exact":
            assert abs(rec.d) <= 1 << 320 and all(x % (1 << 320) == 0 for _, x in rec.pa + rec.na)
        if rec.cls == "top_limbs_zero":
            assert all(x >> 320 == 0 for _, x in rec.pa + rec.na)
    ks = [rec.k for rec in recs[name] if rec.cls == "kp_plus_d"]
    assert min(ks) == -(21 * maxn - 20) and max(ks) == 21 * maxn - 20
    assert any(len(r.pa) + len(r.na) == maxn for r in recs[name] if r.cls == "max_terms")
    assert any(not r.na for r in recs[name]) and any(not r.pa for r in recs[name])


def test_fp12_records(recs):
    """both truth values of the boolean operations are among the records; the cyclotomic elements
    are cyclotomic"""
    from oracle import bls_oracle as o
    assert {r.a == [1] + [0] * 11 for r in recs["r_is_one"]} == {True, False}
    assert {r.a == r.b for r in recs["r_eq"]} == {True, False}
    for rec in recs["r_csqr"]:
        a = V.f12_tower(rec.a)
        assert o.f12_mul(a, o.f12_conj(a)) == V.f12_tower([1] + [0] * 11)  # norm 1 over Fp6 ...
        assert o.f12_mul(o.f12_pow(a, P ** 4), a) == o.f12_pow(a, P * P)     # ... and a^(p^4 - p^2 + 1) = 1
    assert all(any(rec.a) for rec in recs["w_inv"])
    assert [r.chain for r in recs["r_pdbl_fast"]] == [1, 2, V.PDBL_CHAIN] and V.PDBL_CHAIN == 70
