"""The KZG calls under a setup whose tau the tests know (tests/kzg_known_tau.py): every point fed is
[a] G1 with a known, so every expected output is point(one integer mod r), made by the oracle's
group law, and every expected verdict is the scalar model's.  That gives what the ceremony's setup
cannot: exact bytes for DENSE 4096-term sums, proofs and FK20 outputs that do not come from the code
under test, and accepting inputs that pass through the exceptional branches of jac_add_i (equal
terms meeting in k_g1_sum64's tree and in wave_sum64, a doubling in k_kzg_check's
Q = C - [y] G1 + [z] pi, cancellations that leave infinity in one node only).  Which node is which is
checked in integers by tests/test_kzg_known_tau_cpu.py.

The module has an engine of its own, so the session engine's setup is never replaced.  Every
comparison is exact bytes or an exact verdict."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
import kzg_deneb_spec as D  # noqa: E402
import kzg_known_tau as T  # noqa: E402

from lodestar_amd import kzg as K  # noqa: E402

pytestmark = pytest.mark.gpu

R, TAU, INF = T.R, T.TAU, T.INF48
_rnd = random.Random(0x7A0)
POOL = [_rnd.randrange(1, R) for _ in range(16)]          # the given points' logarithms
ORACLE_CHECKED = (0, 1, 63, 64, 127, 2, 65, 126)            # of 128 points from one lb_sk_to_pk launch


@pytest.fixture(scope="module")
def kt():
    """the module's engine under the known-tau setup: (engine, host-mode Kzg, device-mode Kzg)"""
    from lodestar_amd.engine import Engine
    eng = Engine(0)
    setup = T.setup_bin(eng)
    yield eng, K.Kzg(eng, setup=setup), K.Kzg(eng, setup=setup, field="device")
    eng.close()


@pytest.fixture(scope="module")
def host(kt):
    return kt[1]


@pytest.fixture(scope="module")
def dev(kt):
    return kt[2]


@pytest.fixture(scope="module")
def blobs():
    """name -> (coefficients, blob): a dense random polynomial, the geometric one (every term of its
    commitment is the same point) and a dense one with p(TAU) = 0"""
    rnd = random.Random(0xB10B)
    coeffs = {"dense": [rnd.randrange(R) for _ in range(4096)], "geometric": T.geometric_coeffs(rnd.randrange(1, R)),
              "root": T.root_at_tau_coeffs(rnd)}
    return {k: (c, S.coefficients_to_blob(c)) for k, c in coeffs.items()}


def bulk_points(engine, scalars, checked):
    """many points from one lb_sk_to_pk launch, those at `checked` compared with the oracle's"""
    pts = T.engine_points(engine, scalars)
    assert len(checked) >= 8
    for i in checked:
        assert pts[i] == T.point(scalars[i]), f"lb_sk_to_pk point {i}"
    return pts


# ------------------------------------------------------------------ A. lb_g1_lincomb, given points
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097])
def test_lincomb_of_given_points(host, n):
    rnd = random.Random(n)
    pts = [T.point(a) for a in POOL]
    a = [POOL[i % 16] for i in range(n)]
    s = [rnd.randrange(R) for _ in range(n)]
    want = T.point(sum(x * y for x, y in zip(a, s)))
    assert want != INF
    assert host.g1_lincomb(s, [pts[i % 16] for i in range(n)]) == want


@pytest.mark.parametrize("n", [64, 65, 4097])
@pytest.mark.parametrize("kind", T.CRAFTED)
def test_lincomb_of_crafted_terms(host, kind, n):
    """equal terms, cancelling terms and infinities meeting in k_g1_sum64's tree, by name"""
    rnd = random.Random(f"{kind}{n}")
    terms = T.crafted_terms(kind, n, rnd)
    a, s = T.split_terms(kind, terms, POOL, rnd)
    assert host.g1_lincomb(s, [T.point(x) for x in a]) == T.point(sum(terms))


def test_lincomb_edge_scalars(host):
    a = POOL[3]
    for s in (0, 1, 2, R - 1, R - 2, (R - 1) // 2, 1 << 254):
        assert host.g1_lincomb([s], [T.point(a)]) == T.point(a * s), hex(s)
    assert host.g1_lincomb([R - 1], [INF]) == INF
    # [r - 1] P + P and [(r - 1) / 2] P twice + P: cancellations between ladders' results
    assert host.g1_lincomb([R - 1, 1], [T.point(a)] * 2) == INF
    assert host.g1_lincomb([(R - 1) // 2, (R - 1) // 2, 1], [T.point(a)] * 3) == INF


# ------------------------------------------------------------------ B. lb_g1_lincomb, the setup table
def test_setup_lincomb_dense_and_crafted(host):
    rnd = random.Random(0xB)
    dense = [rnd.randrange(R) for _ in range(4096)]
    assert host.g1_lincomb(dense) == T.point(T.commit(dense)) != INF
    a0 = rnd.randrange(1, R)
    assert host.g1_lincomb(T.geometric_coeffs(a0)) == T.point(4096 * a0)     # every addition a doubling
    assert host.g1_lincomb(T.alternating_coeffs(a0)) == INF                   # every block cancels
    assert host.g1_lincomb(T.root_at_tau_coeffs(rnd)) == INF                  # infinity at the root only
    unit = [0] * 4096
    unit[4095] = 1
    assert host.g1_lincomb(unit) == T.point(pow(TAU, 4095, R))


@pytest.mark.parametrize("n", [1, 64, 65, 4095])
def test_setup_lincomb_sizes(host, n):
    rnd = random.Random(n)
    c = [rnd.randrange(R) for _ in range(n)]
    assert host.g1_lincomb(c) == T.point(T.commit(c))
    assert host.g1_lincomb(T.geometric_coeffs(c[0] or 1, n)) == T.point(n * (c[0] or 1))


# ------------------------------------------------------------------ C. blob-level compute, dense references
def _zs(blob_name):
    rnd = random.Random(blob_name)
    return [rnd.randrange(R), D.ROOTS_BRP[1234], TAU]       # random, on the evaluation domain, TAU itself


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("name", ["dense", "geometric", "root"])
def test_blob_commitment_and_proofs(kt, blobs, mode, name):
    kz = kt[2] if mode == "device" else kt[1]
    coeffs, blob = blobs[name]
    c = T.commit(coeffs)
    assert (c == 0) == (name == "root")
    assert kz.blob_to_kzg_commitment(blob) == T.point(c)
    for z in _zs(name):
        y, s = T.blob_proof_scalar(coeffs, z)
        assert kz.compute_kzg_proof_bytes(blob, z.to_bytes(32, "big")) == (T.point(s), y.to_bytes(32, "big")), hex(z)
    commitment = T.point(c)
    _, s = T.blob_proof_scalar(coeffs, D.compute_challenge(blob, commitment))
    assert kz.compute_blob_kzg_proof(blob, commitment) == T.point(s)
    if name == "geometric":
        # the blob proof under a commitment that is not the blob's: another challenge, the same rule
        other = T.point(c + 1)
        _, s = T.blob_proof_scalar(coeffs, D.compute_challenge(blob, other))
        assert kz.compute_blob_kzg_proof(blob, other) == T.point(s)


def _cells_and_proofs(engine, coeffs):
    """(the 128 cells by the Python transform, the 128 proofs [s_k] G1 from one lb_sk_to_pk launch, eight
    of them checked against the oracle)"""
    scalars = [T.cell_proof_scalar(coeffs, k) for k in range(128)]
    return S.compute_cells(coeffs), bulk_points(engine, scalars, ORACLE_CHECKED)


@pytest.fixture(scope="module")
def cellfx(kt, blobs):
    return {name: _cells_and_proofs(kt[0], blobs[name][0]) for name in ("dense", "root")}


@pytest.mark.parametrize("name", ["dense", "root"])
def test_fk20_cells_and_all_proofs(kt, blobs, cellfx, name):
    cells, proofs = cellfx[name]
    for i in ORACLE_CHECKED:
        assert proofs[i] == T.point(T.cell_proof_scalar(blobs[name][0], i))
    got_cells, got_proofs = kt[1].compute_cells_and_kzg_proofs(blobs[name][1])
    assert got_cells == cells
    assert got_proofs == proofs
    assert len(set(proofs)) == 128 and INF not in proofs


@pytest.mark.parametrize("name", ["dense", "geometric", "root"])
def test_direct_cell_proofs(host, blobs, name):
    coeffs, blob = blobs[name]
    assert host.compute_cell_kzg_proofs(blob, [0, 1, 127]) == [T.point(T.cell_proof_scalar(coeffs, k)) for k in (0, 1, 127)]


@pytest.mark.parametrize("have", ["first_half", "odd"])
@pytest.mark.parametrize("name", ["dense", "root"])
def test_recover_cells_and_proofs(kt, blobs, cellfx, name, have):
    cells, proofs = cellfx[name]
    for i in ORACLE_CHECKED:
        assert proofs[i] == T.point(T.cell_proof_scalar(blobs[name][0], i))
    idx = list(range(64)) if have == "first_half" else list(range(1, 128, 2))
    got_cells, got_proofs = kt[1].recover_cells_and_kzg_proofs(idx, [cells[i] for i in idx])
    assert got_cells == cells
    assert got_proofs == proofs


# ------------------------------------------------------------------ D. verify_kzg_proof (k_kzg_check)
POINT_CASES = T.point_check_cases(random.Random(0xD))


@pytest.mark.parametrize("name", sorted(POINT_CASES))
def test_verify_kzg_proof_crafted(host, name):
    """accepting inputs whose Q = (C + (-[y] G1)) + [z] pi passes through a doubling, a cancellation or
    an infinity; each with y + 1 rejects"""
    c, z, y, s = POINT_CASES[name]
    comm, pi = T.point(c), T.point(s)
    assert T.verdict_point(comm, z, y, pi) is True
    assert host.verify_kzg_proof(comm, z, y, pi) is True
    y1 = (y + 1) % R
    assert T.verdict_point(comm, z, y1, pi) is False
    assert host.verify_kzg_proof(comm, z, y1, pi) is False
    if name == "z_is_tau":
        # at z = TAU the check accepts iff C == [y] G1, whatever the proof
        for other in (T.point(s + 1), INF):
            assert host.verify_kzg_proof(comm, z, y, other) is T.verdict_point(comm, z, y, other) is True
        assert host.verify_kzg_proof(T.point(c + 1), z, y, pi) is T.verdict_point(T.point(c + 1), z, y, pi) is False
    if name == "last_doubling":
        # the same doubling under a proof that does not fit: Q = 2 [z s] G1 against pi' = [2 s] G1
        assert host.verify_kzg_proof(comm, z, y, T.point(2 * s)) is T.verdict_point(comm, z, y, T.point(2 * s)) is False


# ------------------------------------------------------------------ E. the batch verifiers
def _forge(engine, blob_list, cs, checked=None):
    """forged accepts: any blob, C_j = [c_j] G1, the proof solved from z_j = H(blob_j, C_j).  blob_list:
    (coefficients, blob) per entry.  Returns (commitments, zs, ys, proofs); the points by the oracle, or
    for long lists from two lb_sk_to_pk launches with `checked` of each compared with the oracle's"""
    make = (lambda sc: [T.point(a) for a in sc]) if checked is None else (lambda sc: bulk_points(engine, sc, checked))
    comms = make(cs)
    zs = [D.compute_challenge(blob, cm) for (_, blob), cm in zip(blob_list, comms)]
    ys = [T.horner(coeffs, z) for (coeffs, _), z in zip(blob_list, zs)]
    proofs = make([(c - y) * T.inv(TAU - z) % R for c, y, z in zip(cs, ys, zs)])
    return comms, zs, ys, proofs


def _check_blob_batch(kz, blob_list, comms, zs, ys, proofs, want):
    assert T.verdict_deneb(comms, zs, ys, proofs) is want
    assert kz.verify_blob_kzg_proof_batch([b for _, b in blob_list], comms, proofs) is want


def test_blob_batch_forged_accepts(kt, blobs):
    eng, host, dev = kt
    rnd = random.Random(0xE1)
    three = [blobs["dense"], blobs["geometric"], blobs["root"]]
    # one blob and two blobs: commitments that are not the blobs', the proofs solved for
    for group in (three[:1], three[:2]):
        comms, zs, ys, proofs = _forge(eng, group, [rnd.randrange(1, R) for _ in group])
        _check_blob_batch(host, group, comms, zs, ys, proofs, True)
        bad = proofs[:-1] + [T.point(T.dlog(proofs[-1]) + 1)]
        _check_blob_batch(host, group, comms, zs, ys, bad, False)
    comms, zs, ys, proofs = _forge(eng, three[:1], [rnd.randrange(1, R)])
    for kz in (host, dev):
        assert kz.verify_blob_kzg_proof(three[0][1], comms[0], proofs[0]) is True
        assert kz.verify_blob_kzg_proof(three[0][1], comms[0], T.point(T.dlog(proofs[0]) * 2)) is False


def test_blob_batch_doubling_in_the_wave_sum(kt):
    """one group of one constant blob v under C = [-v] G1: C + (-[y] G1) is a doubling in wave_sum64
    (lanes 0 and 2 meet at d = 2); accepting with the solved proof, rejecting with twice the proof"""
    eng, host, _ = kt
    v = 0x5EED5EED
    group = [([v], S.values_to_blob([v] * 4096))]
    comms, zs, ys, proofs = _forge(eng, group, [R - v])
    assert ys == [v] and T.dlog(proofs[0]) == (-2 * v) * T.inv(TAU - zs[0]) % R
    _check_blob_batch(host, group, comms, zs, ys, proofs, True)
    _check_blob_batch(host, group, comms, zs, ys, [T.point(2 * T.dlog(proofs[0]))], False)


def test_blob_batch_of_65_forged_accepts(kt, blobs):
    """65 blobs in one group: 131 terms of T and 65 of P, so the per-lane loops run a second pass.  Three
    blobs' bytes under 65 distinct commitments; one changed proof in the middle rejects the group."""
    eng, host, _ = kt
    rnd = random.Random(0xE65)
    three = [blobs["dense"], blobs["geometric"], blobs["root"]]
    group = [three[j % 3] for j in range(65)]
    checked = (0, 1, 2, 31, 32, 63, 64, 40)
    comms, zs, ys, proofs = _forge(eng, group, [rnd.randrange(1, R) for _ in range(65)], checked)
    _check_blob_batch(host, group, comms, zs, ys, proofs, True)
    bad = proofs[:32] + [proofs[33]] + proofs[33:]
    _check_blob_batch(host, group, comms, zs, ys, bad, False)


def test_aggregate_proof_forged_accept(kt, blobs):
    eng, host, dev = kt
    rnd = random.Random(0xA6)
    pair = [blobs["dense"], blobs["geometric"]]
    coeffs, raw = [c for c, _ in pair], [b for _, b in pair]
    comms = [T.point(rnd.randrange(1, R)) for _ in pair]
    c, x, y = T.aggregate_point(coeffs, raw, comms)
    good, bad = T.point((c - y) * T.inv(TAU - x)), T.point((c - y) * T.inv(TAU - x) + 1)
    assert T.verdict_aggregate(coeffs, raw, comms, good) is True and T.verdict_aggregate(coeffs, raw, comms, bad) is False
    for kz in (host, dev):
        assert kz.verify_aggregate_kzg_proof(raw, comms, good) is True
        assert kz.verify_aggregate_kzg_proof(raw, comms, bad) is False
    # one blob: r^0 = 1
    c1, x1, y1 = T.aggregate_point(coeffs[:1], raw[:1], comms[:1])
    good1 = T.point((c1 - y1) * T.inv(TAU - x1))
    assert host.verify_aggregate_kzg_proof_batch([(raw, comms, good), (raw, comms, bad), (raw[:1], comms[:1], good1),
                                                  (raw[:1], comms[:1], good)]) == [True, False, True, False]
    assert T.verdict_aggregate(coeffs[:1], raw[:1], comms[:1], good1) is True
    assert T.verdict_aggregate(coeffs[:1], raw[:1], comms[:1], good) is False


_cell_rnd = random.Random(0xCE11)
CELL_VALS = [_cell_rnd.randrange(R) for _ in range(64)]


@pytest.mark.parametrize("kind", ["plain", "dbl", "cancel", "both_infinity"])
def test_cell_batch_one_cell_groups(host, kind):
    """one-cell groups (r^0 = 1): arbitrary cell values under any C = [c] G1 with the proof solved from
    I(TAU) accept; c chosen so that lane 0's accumulation (the commitment term, then table term 62) is a
    doubling, a cancellation, or so that RL = LL = infinity"""
    idx = 9
    cell = S.values_to_blob(CELL_VALS)
    c, s, _ = T.cell_group_terms(kind, idx, CELL_VALS, random.Random(kind))
    comm, pi = T.point(c), T.point(s)
    assert (pi == INF) == (kind == "both_infinity")
    assert T.verdict_cells([comm], [idx], [cell], [pi]) is True
    assert host.verify_cell_kzg_proof_batch([comm], [idx], [cell], [pi]) is True
    for bad_c, bad_pi in ((comm, T.point(2 * s + 1)), (T.point(c + 1), pi)):
        assert T.verdict_cells([bad_c], [idx], [cell], [bad_pi]) is False
        assert host.verify_cell_kzg_proof_batch([bad_c], [idx], [cell], [bad_pi]) is False


def test_cell_batch_three_cells_two_commitments(host):
    """a 3-cell group over two commitments, forged: every cell's proof solved under its commitment, so
    the group accepts for whatever combiner its bytes hash to; two proofs swapped reject"""
    rnd = random.Random(0xC3)
    ca, cb = rnd.randrange(1, R), rnd.randrange(1, R)
    idx = [0, 127, 64]
    vals = [[rnd.randrange(R) for _ in range(64)] for _ in idx]
    cells = [S.values_to_blob(v) for v in vals]
    cs = [ca, cb, ca]
    comms = [T.point(c) for c in cs]
    proofs = [T.point(T.solve_cell_proof(c, i, v)) for c, i, v in zip(cs, idx, vals)]
    assert T.verdict_cells(comms, idx, cells, proofs) is True
    assert host.verify_cell_kzg_proof_batch(comms, idx, cells, proofs) is True
    swapped = [proofs[2], proofs[1], proofs[0]]
    assert T.verdict_cells(comms, idx, cells, swapped) is False
    assert host.verify_cell_kzg_proof_batch(comms, idx, cells, swapped) is False
    # both verdicts of one call: the forged group beside its reject
    assert host.verify_cell_kzg_proof_batch_many([(comms, idx, cells, proofs), (comms, idx, cells, swapped)]) == [True, False]
