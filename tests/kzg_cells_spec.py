"""Big-integer restatement of the cell proofs of EIP-7594 (the Fulu polynomial-commitments-sampling
spec), for the tests (a helper, not collected).  Independent of lodestar_amd/kzg.py: it builds on
oracle/kzg.py and oracle/bls_oracle.py alone.

    w      = 7^((r - 1) / 8192);  w64 = w^128;  h_i = w^brp7(i)
    cell i = the polynomial's values at roots_brp_8192[64 i .. 64 i + 63] = h_i * w64^brp6(t)
    proof_i = commit(Q_i),  p(X) - I_i(X) = Q_i(X) (X^64 - h_i^64),  deg I_i < 64
    r      = hash_to_bls_field(DOMAIN || 4096 || 64 || #distinct commitments || n || the distinct
             commitments || per cell: commitment index || cell index || cell || proof), integers 8 B BE
    LL     = sum r^k proof_k
    RL     = sum r^k C_k - commit(sum r^k I_k) + sum [r^k h_k^64] proof_k
    accept iff e(LL, [tau^64] G2) e(RL, -G2) == 1;  n = 0 accepts

The transform here is a plain recursive one, the interpolation a direct 64 x 64 inverse DFT and the
quotient a schoolbook long division: none shares a line with the butterflies under test."""
import hashlib

from oracle import bls_oracle as o
from oracle import kzg as OK

R = o.R
N = 4096
EXT = 8192
CELL = 64
CELLS = 128
BYTES_PER_CELL = 32 * CELL
DOMAIN = b"RCKZGCBATCH__V1_"
W = pow(7, (R - 1) // EXT, R)
W64 = pow(W, CELLS, R)
INF48 = bytes([0xC0]) + bytes(47)
ROOTS_BRP = OK.roots_brp(N)


def brp(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def coset_shift(i):
    return pow(W, brp(i, 7), R)


def coset_point(i, t):
    return coset_shift(i) * pow(W64, brp(t, 6), R) % R


def _fft(a, w):
    """recursive transform: out[k] = sum_j a[j] w^(j k)"""
    n = len(a)
    if n == 1:
        return list(a)
    ev, od = _fft(a[0::2], w * w % R), _fft(a[1::2], w * w % R)
    out, x = [0] * n, 1
    for k in range(n // 2):
        t = x * od[k] % R
        out[k] = (ev[k] + t) % R
        out[k + n // 2] = (ev[k] - t) % R
        x = x * w % R
    return out


def blob_values(blob):
    return [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(N)]


def values_to_blob(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def blob_coefficients(blob):
    """monomial coefficients of the polynomial whose values at the bit-reversed roots are the blob"""
    vals = blob_values(blob)
    nat = [0] * N
    for i, v in enumerate(vals):
        nat[brp(i, 12)] = v
    w_inv = pow(pow(W, 2, R), R - 2, R)
    inv_n = pow(N, R - 2, R)
    return [c * inv_n % R for c in _fft(nat, w_inv)]


def coefficients_to_blob(coeffs):
    nat = _fft(list(coeffs) + [0] * (N - len(coeffs)), pow(W, 2, R))
    return values_to_blob(nat[brp(i, 12)] for i in range(N))


def compute_cells(coeffs):
    """the 128 cells (2048 bytes each) of the polynomial with the given coefficients (at most 4096)"""
    nat = _fft(list(coeffs) + [0] * (EXT - len(coeffs)), W)
    ext = [nat[brp(k, 13)] for k in range(EXT)]
    return [values_to_blob(ext[CELL * i: CELL * (i + 1)]) for i in range(CELLS)]


def cell_values(cell):
    return [int.from_bytes(cell[32 * t: 32 * t + 32], "big") for t in range(CELL)]


def horner(coeffs, x):
    y = 0
    for c in reversed(coeffs):
        y = (y * x + c) % R
    return y


def interpolate(cell_index, values):
    """the 64 coefficients of I with I(h w64^brp6(t)) = values[t]: a direct inverse DFT for
    g(Y) = I(h Y), then coefficient j times h^-j"""
    h_inv = pow(coset_shift(cell_index), R - 2, R)
    inv_n = pow(CELL, R - 2, R)
    xs_inv = [pow(W64, (-brp(t, 6)) % CELL, R) for t in range(CELL)]
    out = []
    for j in range(CELL):
        g = sum(values[t] * pow(xs_inv[t], j, R) for t in range(CELL)) % R
        out.append(g * inv_n % R * pow(h_inv, j, R) % R)
    return out


def cell_quotient(coeffs, cell_index):
    """(Q, I) with p = Q (X^64 - h^64) + I by long division; Q has len(coeffs) - 64 coefficients"""
    c = pow(coset_shift(cell_index), CELL, R)
    rem = list(coeffs)
    q = [0] * max(len(rem) - CELL, 0)
    for j in range(len(rem) - 1, CELL - 1, -1):
        q[j - CELL] = rem[j]
        rem[j - CELL] = (rem[j - CELL] + c * rem[j]) % R
        rem[j] = 0
    return q, rem[:CELL]


def dedup(commitments):
    distinct, idx = [], []
    for c in commitments:
        c = bytes(c)
        if c not in distinct:
            distinct.append(c)
        idx.append(distinct.index(c))
    return distinct, idx


def compute_cell_batch_r(commitments, cell_indices, cells, proofs):
    distinct, idx = dedup(commitments)
    data = DOMAIN + N.to_bytes(8, "big") + CELL.to_bytes(8, "big") + len(distinct).to_bytes(8, "big")
    data += len(cells).to_bytes(8, "big") + b"".join(distinct)
    for k in range(len(cells)):
        data += idx[k].to_bytes(8, "big") + int(cell_indices[k]).to_bytes(8, "big") + bytes(cells[k]) + bytes(proofs[k])
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R


def batch_terms(commitments, cell_indices, cells, proofs, setup_g1):
    """the batch equation as two linear combinations: (points, scalars) of LL and of RL"""
    n = len(cells)
    r = compute_cell_batch_r(commitments, cell_indices, cells, proofs)
    pw = [pow(r, k, R) for k in range(n)]
    distinct, idx = dedup(commitments)
    weights = [0] * len(distinct)
    for k in range(n):
        weights[idx[k]] = (weights[idx[k]] + pw[k]) % R
    agg = [0] * CELL
    for k in range(n):
        for j, c in enumerate(interpolate(cell_indices[k], cell_values(cells[k]))):
            agg[j] = (agg[j] + pw[k] * c) % R
    h64 = [pow(coset_shift(i), CELL, R) for i in cell_indices]
    rl_points = distinct + list(setup_g1[:CELL]) + list(proofs)
    rl_scalars = weights + [(-c) % R for c in agg] + [pw[k] * h64[k] % R for k in range(n)]
    return (list(proofs), pw), (rl_points, rl_scalars)


def _jac_double(p):
    x, y, z = p
    a, b = x * x % o.P, y * y % o.P
    c = b * b % o.P
    d = 2 * ((x + b) * (x + b) - a - c) % o.P
    e = 3 * a % o.P
    x3 = (e * e - 2 * d) % o.P
    return x3, (e * (d - x3) - 8 * c) % o.P, 2 * y * z % o.P


def _jac_add_affine(p, q):
    """Jacobian p (z = 0: infinity) plus the affine point q"""
    x1, y1, z1 = p
    if z1 == 0:
        return q[0], q[1], 1
    zz = z1 * z1 % o.P
    h, r = (q[0] * zz - x1) % o.P, (q[1] * z1 * zz - y1) % o.P
    if h == 0:
        return _jac_double(p) if r == 0 else (1, 1, 0)
    hh = h * h % o.P
    hhh, v = h * hh % o.P, x1 * hh % o.P
    x3 = (r * r - hhh - 2 * v) % o.P
    return x3, (r * (v - x3) - y1 * hhh) % o.P, z1 * h % o.P


def _lincomb(points, scalars):
    """sum s_i P_i: one shared run of 255 doublings in Jacobian coordinates (the oracle's affine
    g1_mul point by point takes a second per eight terms), compressed by the oracle"""
    pts = [o.g1_decompress(p48) for p48 in points]
    acc = (1, 1, 0)
    for bit in range(254, -1, -1):
        acc = _jac_double(acc) if acc[2] else acc
        for pt, s in zip(pts, scalars):
            if pt is not None and (s >> bit) & 1:
                acc = _jac_add_affine(acc, pt)
    if acc[2] == 0:
        return o.g1_compress(None)
    zi = o.fp_inv(acc[2])
    return o.g1_compress((acc[0] * zi * zi % o.P, acc[1] * zi * zi * zi % o.P))


def pairing_product(ll48, rl48, setup_g2):
    """e(LL, [tau^64] G2) e(RL, -G2) == 1 in pure Python"""
    ll, rl = o.g1_decompress(ll48), o.g1_decompress(rl48)
    f = o.F12_ONE
    if ll is not None:
        f = o.f12_mul(f, o.miller_loop(ll, o.g2_decompress(setup_g2[64])))
    if rl is not None:
        f = o.f12_mul(f, o.miller_loop(rl, o.g2_neg(o.g2_decompress(setup_g2[0]))))
    return o.final_exponentiation(f) == o.F12_ONE


def batch_equation(commitments, cell_indices, cells, proofs, setup_g1, setup_g2, lincomb=_lincomb):
    if not cells:
        return True
    (lp, ls), (rp, rs) = batch_terms(commitments, cell_indices, cells, proofs, setup_g1)
    return bool(pairing_product(lincomb(lp, ls), lincomb(rp, rs), setup_g2))
