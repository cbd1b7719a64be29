"""The known-tau helper (tests/kzg_known_tau.py) kept honest without a GPU: TAU is a usable tau, the
scalar model's verdicts agree with the pure-Python pairing on a degree-3 polynomial (one honest
accept, one forged accept, one reject), and every crafted input of tests/test_kzg_known_tau_gpu.py
has, in integers, the property it is named for: which additions of the device's trees are
doublings, which cancel, where the sum first becomes infinity.  The trees are restated in Python
(lane t takes lane t + d, d = 32 .. 1; 64 : 1 per level; the check kernels' lane q % 64 loop)."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
import kzg_deneb_spec as D  # noqa: E402
import kzg_known_tau as T  # noqa: E402

from oracle import bls_oracle as o  # noqa: E402
from oracle import kzg as OK  # noqa: E402

R, TAU = T.R, T.TAU


def test_tau_is_usable():
    assert 1 < TAU < R
    assert pow(TAU, 8192, R) != 1                       # TAU is on neither evaluation domain
    h64 = {pow(S.coset_shift(k), 64, R) for k in range(128)}
    assert len(h64) == 128 and T.TAU64 not in h64       # every cell's X^64 - h^64 is invertible at TAU
    assert TAU * T.inv(2) % R != 0 and 2 * TAU % R != 0
    assert TAU * T.TAU_INV % R == 1
    pw = T.tau_powers()
    assert len(pw) == 4096 and pw[0] == 1 and pw[1] == TAU and pw[4095] == pow(TAU, 4095, R)


def test_point_is_the_oracles_multiple_and_dlog_inverts_it():
    rnd = random.Random(1)
    for a in (1, 2, 15, 16, 17, R - 1, R - 2, (R - 1) // 2, 1 << 254, TAU, rnd.randrange(R)):
        assert T.point(a) == o.g1_compress(o.g1_mul(o.G1, a % R)), a
        assert T.dlog(T.point(a)) == a % R
    assert T.point(0) == T.INF48 == T.point(R) and T.dlog(T.INF48) == 0
    assert T.dlog(("tau", 3)) == pow(TAU, 3, R)
    with pytest.raises(KeyError):
        T.dlog(o.g1_compress(o.g1_mul(o.G1, 0xABCDEF123)))   # a point the helper did not make


def test_setup_g2_pairs_with_tau():
    g2 = T.setup_g2()
    assert len(g2) == 65 and g2[0] == g2[2] == g2[63]
    with open(T.SHIPPED_SETUP, "rb") as f:
        assert g2[0] == f.read()[8 + 4096 * 48:][:96]
    gen = o.g2_decompress(g2[0])
    t1 = o.g1_decompress(T.point(TAU))
    assert o.pairing(t1, gen) == o.pairing(o.G1, o.g2_decompress(g2[1]))
    assert o.g2_decompress(g2[64]) == o.g2_mul(o.g2_decompress(g2[1]), pow(TAU, 63, R))


def test_verdicts_agree_with_the_pure_python_pairing():
    """degree 3: the setup points it needs by the oracle; an honest accept, a forged accept (a
    commitment that is not the blob's, the proof solved for) and a reject, through verdict_deneb /
    kzg_deneb_spec.batch_equation and verdict_point / OK.verify_kzg_proof_impl"""
    g2 = T.setup_g2()
    coeffs = [5, 0, R - 3, 11]
    blob = D.low_degree_blob(coeffs)
    setup_g1 = [T.point(pow(TAU, i, R)) for i in range(4)]
    _, comm, z, y, proof = D.low_degree_proof(setup_g1, coeffs)
    assert comm == T.point(T.commit(coeffs))
    want_y, s = T.blob_proof_scalar(coeffs, z)
    assert (y, proof) == (want_y, T.point(s))
    # forged: C = [c] G1 for any c, z from the transcript, the proof solved from c = y + s (TAU - z)
    c = 0xF0F0F0F0F0
    forged_c = T.point(c)
    fz = D.compute_challenge(blob, forged_c)
    fy = T.horner(coeffs, fz)
    forged_pi = T.point((c - fy) * T.inv(TAU - fz))
    cases = [([comm], [z], [y], [proof], True), ([forged_c], [fz], [fy], [forged_pi], True),
             ([comm], [z], [(y + 1) % R], [proof], False), ([comm, forged_c], [z, fz], [y, fy], [proof, forged_pi], True),
             ([comm, forged_c], [z, fz], [y, fy], [forged_pi, proof], False)]
    for cm, zs, ys, pf, want in cases:
        assert T.verdict_deneb(cm, zs, ys, pf) is want
        assert D.batch_equation(cm, zs, ys, pf, g2) is want
    for cm, zz, yy, pf, want in [(comm, z, y, proof, True), (forged_c, fz, fy, forged_pi, True), (comm, z, y, forged_pi, False)]:
        assert T.verdict_point(cm, zz, yy, pf) is want
        assert bool(OK.verify_kzg_proof_impl(cm, zz, yy, pf, g2)) is want
    # z = TAU: accepts iff C == [y] G1, whatever the proof
    assert T.verdict_point(T.point(77), TAU, 77, proof) is True and T.verdict_point(T.point(78), TAU, 77, proof) is False
    assert T.verdict_deneb([], [], [], []) is True and T.verdict_cells([], [], [], []) is True


def test_proof_scalars_agree_with_division():
    rnd = random.Random(2)
    coeffs = [rnd.randrange(R) for _ in range(200)]
    z = rnd.randrange(R)
    y, q = D.synthetic_division(coeffs, z)
    assert T.blob_proof_scalar(coeffs, z) == (y, T.commit(q))
    yt, qt = D.synthetic_division(coeffs, TAU)
    assert T.blob_proof_scalar(coeffs, TAU) == (yt, T.commit(qt)) and yt == T.commit(coeffs)
    deriv = sum(i * c * pow(TAU, i - 1, R) for i, c in enumerate(coeffs) if i) % R
    assert T.commit(qt) == deriv                         # the quotient at its own point: p'(TAU)
    for k in (0, 1, 127):
        qk, ik = S.cell_quotient(coeffs, k)
        assert T.cell_proof_scalar(coeffs, k) == T.commit(qk)
        # a one-cell group under the polynomial's own commitment: the solved proof is the cell's proof
        vals = [T.horner(coeffs, S.coset_point(k, t)) for t in range(64)]
        assert S.interpolate(k, vals) == ik
        assert T.solve_cell_proof(T.commit(coeffs), k, vals) == T.commit(qk)


def test_cell_verdict_model():
    """a one-cell group's scalars are the test's to choose (r^0 = 1): arbitrary values, any c, the proof
    solved; two further cells make a 3-cell group over two commitments whose verdict is the model's"""
    rnd = random.Random(3)
    vals = [rnd.randrange(R) for _ in range(64)]
    cell = S.values_to_blob(vals)
    c = rnd.randrange(R)
    s = T.solve_cell_proof(c, 9, vals)
    assert T.verdict_cells([T.point(c)], [9], [cell], [T.point(s)]) is True
    assert T.verdict_cells([T.point(c)], [9], [cell], [T.point(2 * s)]) is False
    assert T.verdict_cells([T.point(c + 1)], [9], [cell], [T.point(s)]) is False
    # RL = LL = infinity: the commitment is [I(TAU)] G1 and the proof infinity
    i_tau = T.horner(S.interpolate(9, vals), TAU)
    assert T.solve_cell_proof(i_tau, 9, vals) == 0
    assert T.verdict_cells([T.point(i_tau)], [9], [cell], [T.INF48]) is True


# ------------------------------------------------------------------ the crafted inputs' own properties
SIZES = (64, 65, 4097)


def _kinds(levels):
    return [k for blocks in levels for ev in blocks for k in ev.values()]


@pytest.mark.parametrize("n", SIZES)
def test_crafted_lincomb_terms_have_their_properties(n):
    rnd = random.Random(n)
    full = n // 64                                            # full blocks of the first level
    # all equal: every addition inside a full block is a doubling, at every level that has full blocks
    t = T.crafted_terms("all_equal", n, rnd)
    total, levels = T.lincomb_tree(t)
    assert total == n * t[0] % R
    assert all(k == "dbl" for b in range(full) for k in levels[0][b].values())
    if n == 4097:
        assert all(k == "dbl" for k in levels[1][0].values()) and levels[2][0][(0, 1)] == "add"
    assert "cancel" not in _kinds(levels)
    # alternating: lanes t and t + d double down to d = 2, lanes 0 and 1 cancel: every full block is infinity
    t = T.crafted_terms("alternate", n, rnd)
    total, levels = T.lincomb_tree(t)
    for b in range(full):
        ev = levels[0][b]
        assert all(k == "dbl" for (lo, hi), k in ev.items() if hi - lo >= 2) and ev[(0, 1)] == "cancel"
        assert T.sum64(t[64 * b: 64 * b + 64])[0] == 0
    assert total == (t[0] if n % 2 else 0)
    # one doubling, in node (0, 32) of block 0, nothing else exceptional
    t = T.crafted_terms("one_doubling", n, rnd)
    total, levels = T.lincomb_tree(t)
    assert levels[0][0][(0, 32)] == "dbl" and _kinds(levels).count("dbl") == 1 and "cancel" not in _kinds(levels)
    assert total == sum(t) % R != 0
    # one cancellation, in node (0, 1) of block 0
    t = T.crafted_terms("one_cancel", n, rnd)
    total, levels = T.lincomb_tree(t)
    assert levels[0][0][(0, 1)] == "cancel" and _kinds(levels).count("cancel") == 1 and "dbl" not in _kinds(levels)
    assert total == sum(t) % R and (total == 0) == (n == 64)
    # infinity only at the top of the last level
    t = T.crafted_terms("top_infinity", n, rnd)
    total, levels = T.lincomb_tree(t)
    assert total == 0 and levels[-1][0][(0, 1)] == "cancel" and _kinds(levels).count("cancel") == 1
    assert "dbl" not in _kinds(levels)
    # infinity inputs under non-zero scalars, lanes 0 and 32 of block 0 among them; every scalar zero
    pool = [rnd.randrange(1, R) for _ in range(16)]
    t = T.crafted_terms("infinity_inputs", n, rnd)
    a, s = T.split_terms("infinity_inputs", t, pool, rnd)
    assert t[0] == t[32] == t[3] == 0 and all(s) and all((x == 0) == (y == 0) for x, y in zip(a, t))
    assert T.lincomb_tree(t)[1][0][0][(0, 32)] == "inf" and [x * y % R for x, y in zip(a, s)] == t
    t = T.crafted_terms("zero_scalars", n, rnd)
    a, s = T.split_terms("zero_scalars", t, pool, rnd)
    assert not any(s) and all(a) and T.lincomb_tree(t)[0] == 0
    for kind in ("all_equal", "one_cancel"):
        t = T.crafted_terms(kind, n, rnd)
        a, s = T.split_terms(kind, t, pool, rnd)
        assert [x * y % R for x, y in zip(a, s)] == t and len(set(a)) == 16


def test_crafted_setup_vectors_have_their_properties():
    pw = T.tau_powers()
    rnd = random.Random(4)
    a0 = rnd.randrange(1, R)
    geo = T.geometric_coeffs(a0)
    terms = [c * p % R for c, p in zip(geo, pw)]
    assert set(terms) == {a0}                                 # all 4096 terms are the same point
    total, levels = T.lincomb_tree(terms)
    assert total == 4096 * a0 % R == T.commit(geo) and set(_kinds(levels)) == {"dbl"}
    alt = T.alternating_coeffs(a0)
    terms = [c * p % R for c, p in zip(alt, pw)]
    assert terms[:2] == [a0, R - a0] and T.commit(alt) == 0
    total, levels = T.lincomb_tree(terms)
    assert total == 0 and all(ev[(0, 1)] == "cancel" for ev in levels[0])
    root = T.root_at_tau_coeffs(rnd)
    terms = [c * p % R for c, p in zip(root, pw)]
    total, levels = T.lincomb_tree(terms)
    assert total == 0 == T.commit(root) and _kinds(levels).count("cancel") == 1 and levels[1][0][(0, 1)] == "cancel"
    assert "dbl" not in _kinds(levels) and "inf" not in _kinds(levels)


def test_crafted_point_checks_have_their_properties():
    """k_kzg_check's Q = (C + (-[y] G1)) + [z] pi: which of the two additions is a doubling"""
    rnd = random.Random(5)
    for name, (c, z, y, s) in T.point_check_cases(rnd).items():
        assert (c - y) % R == (TAU - z) * s % R, name          # every case accepts
        assert (c - (y + 1)) % R != (TAU - z) * s % R
        first, last = T.classify(c, -y), T.classify(c - y, z * s)
        if name == "last_doubling":
            assert z == TAU * T.inv(2) % R and last == "dbl" and first == "add"
        elif name == "first_doubling":
            assert c == R - y and first == "dbl" and last == "add"
        elif name == "z_is_tau":
            assert z == TAU and c == y and first == "cancel"
        elif name == "z_zero":
            assert z == 0 and last == "inf"
        elif name == "y_zero":
            assert y == 0 and first == "inf"
        elif name == "y_r_minus_1":
            assert y == R - 1
        else:
            assert name == "random" and (first, last) == ("add", "add")


def test_crafted_batch_groups_have_their_properties():
    rnd = random.Random(6)
    # one-blob group, constant blob v, C = [-v] G1: wave_sum64 meets C (lane 0) and -[y] G1 (lane 2) at d = 2
    v, z = rnd.randrange(1, R), rnd.randrange(R)
    c, y = R - v, v
    s = (c - y) * T.inv(TAU - z) % R
    lanes, _ = T.lane_loop([c, z * s % R, R - y])
    assert T.sum64(lanes)[1][(0, 2)] == "dbl"
    assert (c + z * s - y) % R == TAU * s % R
    # 65 blobs: 131 terms of T, a second and a third pass of the per-lane loop; 65 terms of P, a second pass
    assert len(T.lane_loop([1] * 131)[1]) == 131 - 64 and len(T.lane_loop([1] * 65)[1]) == 1
    # a one-cell group: lane 0 adds the commitment term (q = 0) and table term 62 (q = 64)
    vals = [rnd.randrange(R) for _ in range(64)]
    for kind, want in (("dbl", "dbl"), ("cancel", "cancel"), ("plain", "add")):
        c, s, terms = T.cell_group_terms(kind, 9, vals, rnd)
        lanes, ev = T.lane_loop(terms)
        assert len(terms) == 66 and ev[64] == want and ev[65] == "add", kind
        assert sum(terms) % R == T.TAU64 * s % R                  # RL = [tau^64] LL: accepts
    c, s, terms = T.cell_group_terms("both_infinity", 9, vals, rnd)
    assert s == 0 and sum(terms) % R == 0
