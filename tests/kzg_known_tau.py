"""A trusted setup whose tau the tests know, and the scalar model that goes with it (a helper, not
collected).  With the ceremony's setup nobody knows tau, so a dense expected commitment can only be
another GPU result.  Here every point a test feeds is [a] G1 with a known: every expected output
is one integer mod r, every expected verdict is `t == TAU * p` (or `TAU^64 * p`), and a test can
choose its scalars so that any chosen addition of the device's sums is a doubling or a cancellation
while the input still accepts.

Everything below is plain integer arithmetic over oracle/ and the spec restatements
(kzg_deneb_spec.py, kzg_cells_spec.py); nothing comes from lodestar_amd/kzg.py's field code.  The
setup exists only in the tests: `Kzg(engine, setup=setup_bin(engine))` on an engine of the test's own."""
import hashlib
import os
import struct

import kzg_cells_spec as S
import kzg_deneb_spec as D

from oracle import bls_oracle as o
from oracle import kzg as OK

R = o.R
N = 4096
INF48 = bytes([0xC0]) + bytes(47)
TAU = int.from_bytes(hashlib.sha256(b"lodestar-amd tests: known-tau KZG setup").digest(), "big") % R
TAU_INV = pow(TAU, R - 2, R)
TAU64 = pow(TAU, 64, R)
SHIPPED_SETUP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lodestar_amd", "trusted_setup.bin")


def inv(a):
    a %= R
    assert a, "inverse of zero"
    return pow(a, R - 2, R)


def tau_powers(n=N):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * TAU % R
    return out


# ------------------------------------------------------------------ points with known logarithms
# [a] G1 by the oracle's group law alone: a fixed-base table of the generator's multiples
# d * 16^w G1 (d = 1 .. 15, built with o.g1_add) and one o.g1_add per non-zero hex digit of a,
# a sixth of the time of o.g1_mul's double-and-add (which test_kzg_known_tau_cpu.py checks it against).
_WINDOWS = None
_DLOG = {INF48: 0}
_POINT = {}


def _windows():
    global _WINDOWS
    if _WINDOWS is None:
        tab, base = [], o.G1
        for _ in range(64):
            row, acc = [None], None
            for _ in range(15):
                acc = o.g1_add(acc, base)
                row.append(acc)
            tab.append(row)
            base = o.g1_add(acc, base)   # 16 * base
        _WINDOWS = tab
    return _WINDOWS


def point(a):
    """the 48 compressed bytes of [a mod r] G1; a = 0 gives the point at infinity"""
    a %= R
    if a == 0:
        return INF48
    if a in _POINT:
        return _POINT[a]
    tab, acc, k, w = _windows(), None, a, 0
    while k:
        if k & 15:
            acc = o.g1_add(acc, tab[w][k & 15])
        k >>= 4
        w += 1
    b = o.g1_compress(acc)
    _DLOG[b] = a
    _POINT[a] = b
    return b


def register(points48, scalars):
    """points of known logarithm that another route produced (one lb_sk_to_pk launch); the caller
    checks a sample of them against point()"""
    for p, a in zip(points48, scalars):
        _DLOG[bytes(p)] = a % R


def engine_points(engine, scalars):
    """[a] G1 for many a in one lb_sk_to_pk launch (a = 0: infinity, which no secret key is)"""
    live = [a % R for a in scalars if a % R]
    got = iter(bytes(row) for row in engine.sk_to_pk(live)[0]) if live else iter(())
    out = [next(got) if a % R else INF48 for a in scalars]
    register(out, scalars)
    return out


def dlog(p):
    """a for the bytes of a point this helper produced; ("tau", j) stands for the setup's [TAU^j] G1"""
    if isinstance(p, tuple):
        return pow(TAU, p[1], R)
    return _DLOG[bytes(p)]


# ------------------------------------------------------------------ the setup
def shipped_g2_generator():
    with open(SHIPPED_SETUP, "rb") as f:
        data = f.read()
    base = 8 + N * 48
    return o.g2_decompress(data[base: base + 96])


def setup_g2():
    """65 compressed G2 points: [TAU^0], [TAU^1] and [TAU^64] G2 where lb_kzg_load_setup reads them, the
    generator in every other slot"""
    g = shipped_g2_generator()
    gen = o.g2_compress(g)
    out = [gen] * 65
    out[1] = o.g2_compress(o.g2_mul(g, TAU))
    out[64] = o.g2_compress(o.g2_mul(g, TAU64))
    return out


def setup_bin(engine):
    """the known-tau setup in trusted_setup.bin's layout: the 4096 [TAU^i] G1 from one lb_sk_to_pk
    launch, entries 0, 1, 2, 64 and 4095 checked against the oracle's double-and-add"""
    pw = tau_powers()
    g1 = engine_points(engine, pw)
    for i in (0, 1, 2, 64, 4095):
        assert g1[i] == o.g1_compress(o.g1_mul(o.G1, pw[i])), f"setup G1 entry {i}"
    g2 = setup_g2()
    return struct.pack(">II", N, 65) + b"".join(g1) + b"".join(g2)


# ------------------------------------------------------------------ the scalar model
def horner(coeffs, x):
    return S.horner(coeffs, x)


def commit(coeffs):
    """the logarithm of the commitment: sum c_i TAU^i"""
    return horner(coeffs, TAU)


def blob_proof_scalar(coeffs, z):
    """(y, s): y = p(z) and the logarithm of the proof, (p(TAU) - y) / (TAU - z); at z = TAU the
    quotient's own value, p'(TAU), by synthetic division"""
    z %= R
    y = horner(coeffs, z)
    if z == TAU:
        y2, q = D.synthetic_division(list(coeffs), z)
        assert y2 == y
        return y, horner(q, TAU)
    return y, (commit(coeffs) - y) * inv(TAU - z) % R


def cell_interpolant(coeffs, k):
    """the 64 coefficients of I_k = p mod (X^64 - h_k^64)"""
    return S.cell_quotient(list(coeffs), k)[1]


def cell_proof_scalar(coeffs, k):
    """(p(TAU) - I_k(TAU)) / (TAU^64 - h_k^64)"""
    h64 = pow(S.coset_shift(k), 64, R)
    return (commit(coeffs) - horner(cell_interpolant(coeffs, k), TAU)) * inv(TAU64 - h64) % R


def solve_cell_proof(c, cell_index, cell_vals):
    """the proof's logarithm that makes a one-cell group accept under the commitment [c] G1, whatever the
    cell's 64 values are: (c - I(TAU)) / (TAU^64 - h^64) with I the cell's interpolant"""
    h64 = pow(S.coset_shift(cell_index), 64, R)
    return (c - horner(S.interpolate(cell_index, list(cell_vals)), TAU)) * inv(TAU64 - h64) % R


def _lin(points, scalars):
    return sum(dlog(p) * s for p, s in zip(points, scalars)) % R


def verdict_deneb(commitments, zs, ys, proofs):
    """verify_blob_kzg_proof_batch's verdict: kzg_deneb_spec.batch_terms with every point replaced by
    its logarithm, e(T, -G2) e(P, [tau] G2) == 1 iff t == TAU * p"""
    if not commitments:
        return True
    (tp, ts), (pp, ps) = D.batch_terms(list(commitments), list(zs), list(ys), list(proofs))
    return _lin(tp, ts) == TAU * _lin(pp, ps) % R


def verdict_cells(commitments, cell_indices, cells, proofs):
    """verify_cell_kzg_proof_batch's verdict: kzg_cells_spec.batch_terms in logarithms,
    e(LL, [tau^64] G2) e(RL, -G2) == 1 iff rl == TAU^64 * ll"""
    if not cells:
        return True
    tau_points = [("tau", j) for j in range(64)]
    (lp, ls), (rp, rs) = S.batch_terms(list(commitments), list(cell_indices), list(cells), list(proofs), tau_points)
    return _lin(rp, rs) == TAU64 * _lin(lp, ls) % R


def verdict_point(commitment, z, y, proof):
    """verify_kzg_proof's verdict: e(C - [y] G1, -G2) e(pi, [tau - z] G2) == 1 iff c - y == (TAU - z) s"""
    return (dlog(commitment) - y) % R == (TAU - z) * dlog(proof) % R


def aggregate_point(blob_coeffs, blobs, commitments):
    """(c, x, y) of verify_aggregate_kzg_proof: the transcript's powers of r and x over the blobs' values
    (oracle/kzg.py compute_challenges), c = sum r^j c_j, y = sum r^j p_j(x)"""
    polys = [D.blob_values(b) for b in blobs]
    pw, x = OK.compute_challenges(polys, [bytes(c) for c in commitments])
    c = sum(w * dlog(cm) for w, cm in zip(pw, commitments)) % R
    y = sum(w * horner(cf, x) for w, cf in zip(pw, blob_coeffs)) % R
    return c, x, y


def verdict_aggregate(blob_coeffs, blobs, commitments, proof):
    c, x, y = aggregate_point(blob_coeffs, blobs, commitments)
    return (c - y) % R == (TAU - x) * dlog(proof) % R


# ------------------------------------------------------------------ the device's addition order, in logarithms
def classify(a, b):
    """what jac_add_i does with [a] G1 + [b] G1"""
    a, b = a % R, b % R
    if a == 0 or b == 0:
        return "inf"
    if a == b:
        return "dbl"
    if (a + b) % R == 0:
        return "cancel"
    return "add"


def sum64(terms):
    """k_g1_sum64 / wave_sum64 over up to 64 logarithms (missing lanes hold infinity): lane t takes lane
    t + d for d = 32, 16, 8, 4, 2, 1.  Returns (lane 0's sum, {(t, t + d): kind of addition})"""
    v = [t % R for t in terms] + [0] * (64 - len(terms))
    assert len(v) == 64
    events = {}
    for d in (32, 16, 8, 4, 2, 1):
        for t in range(d):
            events[(t, t + d)] = classify(v[t], v[t + d])
            v[t] = (v[t] + v[t + d]) % R
    return v[0], events


def lincomb_tree(terms):
    """lb_g1_lincomb's reduction: 64 : 1 per level until one sum is left.  Returns (the sum, one list
    per level of the blocks' event tables)"""
    cur, levels = [t % R for t in terms], []
    while len(cur) > 1:
        blocks = [sum64(cur[i: i + 64]) for i in range(0, len(cur), 64)]
        levels.append([ev for _, ev in blocks])
        cur = [s for s, _ in blocks]
    return (cur[0] if cur else 0), levels


def lane_loop(terms):
    """the check kernels' accumulation before wave_sum64: lane q % 64 adds term q in order.  Returns
    (the 64 lanes' sums, {q: kind of addition} for the passes after the first)"""
    v, events = [0] * 64, {}
    for q, t in enumerate(terms):
        if q >= 64:
            events[q] = classify(v[q % 64], t)
        v[q % 64] = (v[q % 64] + t) % R
    return v, events


# ------------------------------------------------------------------ crafted coefficient vectors over the setup table
def geometric_coeffs(a0, n=N):
    """a_i = a0 TAU^-i: every term a_i [TAU^i] G1 is the same point [a0] G1, every addition a doubling"""
    out, x = [], a0 % R
    for _ in range(n):
        out.append(x)
        x = x * TAU_INV % R
    return out


def alternating_coeffs(a0, n=N):
    """(-1)^i a0 TAU^-i: the terms alternate [a0] G1, -[a0] G1"""
    return [c if i % 2 == 0 else (R - c) % R for i, c in enumerate(geometric_coeffs(a0, n))]


def root_at_tau_coeffs(rnd, n=N):
    """a dense vector with a_0 adjusted so that p(TAU) = 0: the sum is infinity only at its root"""
    c = [rnd.randrange(1, R) for _ in range(n)]
    c[0] = (c[0] - commit(c)) % R
    return c


def point_check_cases(rnd):
    """accepting inputs (c, z, y, s) of verify_kzg_proof, C = [c] G1 and pi = [s] G1 with
    c = y + s (TAU - z), named for what k_kzg_check's Q = (C + (-[y] G1)) + [z] pi meets"""
    def solve_c(z, y, s):
        return (y + s * (TAU - z)) % R

    out = {}
    z, y, s = rnd.randrange(R), rnd.randrange(R), rnd.randrange(1, R)
    out["random"] = (solve_c(z, y, s), z, y, s)
    z, y, s = TAU * inv(2) % R, rnd.randrange(R), rnd.randrange(1, R)
    out["last_doubling"] = (solve_c(z, y, s), z, y, s)         # c - y = s TAU / 2 = z s
    z, y = rnd.randrange(R), rnd.randrange(1, R)
    out["first_doubling"] = (R - y, z, y, (-2 * y) * inv(TAU - z) % R)   # c = -y
    y, s = rnd.randrange(1, R), rnd.randrange(1, R)
    out["z_is_tau"] = (y, TAU, y, s)                           # accepts iff c == y, whatever s
    y, s = rnd.randrange(1, R), rnd.randrange(1, R)
    out["z_zero"] = (solve_c(0, y, s), 0, y, s)
    z, s = rnd.randrange(R), rnd.randrange(1, R)
    out["y_zero"] = (solve_c(z, 0, s), z, 0, s)
    z, s = rnd.randrange(R), rnd.randrange(1, R)
    out["y_r_minus_1"] = (solve_c(z, R - 1, s), z, R - 1, s)
    return out


def cell_group_terms(kind, cell_index, cell_vals, rnd):
    """(c, s, RL's 66 term logarithms in k_kzg_check_cells' order) of an accepting one-cell group: the
    commitment term (weight r^0 = 1), [h^64] pi, then the table terms -I_j [TAU^j] G1, j = 0 .. 63.
    Lane q % 64 adds term q, so lane 0 adds the commitment term and then table term 62.  `kind`: "dbl"
    makes that addition a doubling, "cancel" a cancellation, "plain" neither; "both_infinity" is
    c = I(TAU) with the proof at infinity (RL = LL = infinity)."""
    interp = S.interpolate(cell_index, list(cell_vals))
    table = [(-interp[j]) * pow(TAU, j, R) % R for j in range(64)]
    assert table[62]
    c = {"dbl": table[62], "cancel": (-table[62]) % R, "plain": rnd.randrange(1, R),
         "both_infinity": horner(interp, TAU)}[kind]
    s = solve_cell_proof(c, cell_index, cell_vals)
    h64 = pow(S.coset_shift(cell_index), 64, R)
    return c, s, [c, h64 * s % R] + table


# ------------------------------------------------------------------ crafted term lists for lb_g1_lincomb
CRAFTED = ("all_equal", "alternate", "one_doubling", "one_cancel", "top_infinity", "infinity_inputs", "zero_scalars")


def crafted_terms(kind, n, rnd):
    """n term logarithms t_i (term i is [t_i] G1) with the property `kind` names; test_kzg_known_tau_cpu.py
    checks each property on the tree model.  "infinity_inputs" and "zero_scalars" also need the split
    into point and scalar, see split_terms."""
    t = [rnd.randrange(1, R) for _ in range(n)]
    if kind == "all_equal":
        t = [t[0]] * n
    elif kind == "alternate":
        t = [t[0] if i % 2 == 0 else R - t[0] for i in range(n)]
    elif kind == "one_doubling":
        t[32] = t[0]
    elif kind == "one_cancel":
        # lane 0 meets lane 1 last, holding the even and the odd lanes' sums of block 0
        t[1] = -(sum(t[0:64:2]) + sum(t[3:64:2])) % R
    elif kind == "top_infinity":
        t[n - 1] = -sum(t[: n - 1]) % R
    elif kind == "infinity_inputs":
        for i in range(n):
            if i % 7 == 3 or i in (0, 32, n - 1):
                t[i] = 0
    elif kind == "zero_scalars":
        t = [0] * n
    else:
        raise ValueError(kind)
    return t


def split_terms(kind, terms, pool, rnd):
    """(point logarithms a_i, scalars s_i) with a_i s_i = t_i: the points cycle through `pool` (a few
    logarithms whose points the oracle made).  A zero term is an infinity point under a non-zero
    scalar, or for "zero_scalars" a finite point under the scalar 0."""
    a, s = [], []
    for i, t in enumerate(terms):
        if t == 0 and kind != "zero_scalars":
            a.append(0)
            s.append(rnd.randrange(1, R))
        else:
            a.append(pool[i % len(pool)])
            s.append(t * inv(a[-1]) % R)
    return a, s
