"""Big-integer restatement of cell recovery (EIP-7594 recover_cells_and_kzg_proofs' scalar-field half),
for the tests (a helper, not collected).  It builds on tests/kzg_cells_spec.py alone.  Two routes from
a blob's given cells to its 4096 coefficients:

  (a) recover_spec: the consensus spec taken literally: the vanishing polynomial of the missing cells
      with stride 64 (sum_k zc[k] X^(64 k)), E Z over the 8192-point domain, coset shift 7, division,
      the first 4096 coefficients.
  (b) recover_columns: what lb_kzg_recover_cells_and_proofs runs (lodestar_amd/csrc/lb_recover.h): with
      p(X) = sum_{r < 64} X^r P_r(X^64), coefficient r of cell i's interpolation polynomial is
      P_r(w128^brp7(i)); per column r one erasure decode of size 128 with Z(Y) = prod over missing
      cells of (Y - w128^brp7(i)) and the shift s = W.  Output k < 64 of column r is coefficient
      64 k + r; the outputs 64 .. 127 ("upper half") are all zero exactly when the given cells lie on
      one polynomial of degree < 4096."""
import kzg_cells_spec as S

R = S.R
N = S.N
W128 = pow(S.W, 64, R)
SHIFT = S.W                      # s: s^128 = W64 != 1
SPEC_SHIFT = 7                   # the spec's PRIMITIVE_ROOT_OF_UNITY as coset shift


def inv(x):
    return pow(x, R - 2, R)


def inv_all(xs):
    """the inverses of non-zero values with one exponentiation (Montgomery's trick)"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    acc, out = inv(acc), [0] * len(xs)
    for k in range(len(xs) - 1, -1, -1):
        out[k] = acc * pre[k] % R
        acc = acc * xs[k] % R
    return out


def scale_by_powers(poly, f):
    """coefficient k times f^k"""
    out, x = [], 1
    for c in poly:
        out.append(c * x % R)
        x = x * f % R
    return out


def point(cell):
    """cell i's point is W128^point(i)"""
    return S.brp(cell, 7)


def _ifft(vals, w):
    n_inv = inv(len(vals))
    return [v * n_inv % R for v in S._fft(list(vals), inv(w))]


def _poly_from_roots(roots):
    p = [1]
    for x in roots:
        q = [0] * (len(p) + 1)
        for k, c in enumerate(p):
            q[k + 1] = (q[k + 1] + c) % R
            q[k] = (q[k] - c * x) % R
        p = q
    return p


def vanishing(cell_indices):
    """coefficients of Z(Y), lowest first"""
    present = set(cell_indices)
    return _poly_from_roots([pow(W128, point(i), R) for i in range(S.CELLS) if i not in present])


def zero_values(cell_indices):
    """(Zev, 1 / Zc): Z at W128^m and the inverse of Z at SHIFT W128^m, m < 128"""
    z = vanishing(cell_indices)
    zev = [S.horner(z, pow(W128, m, R)) for m in range(S.CELLS)]
    zcinv = [inv(S.horner(z, SHIFT * pow(W128, m, R) % R)) for m in range(S.CELLS)]
    return zev, zcinv


def interpolate(cell_index, values):
    """S.interpolate by a 64-point inverse transform instead of its 4096 powers (the CPU test holds
    the two against each other): g(Y) = I(h Y) from the values un-reversed, then coefficient j times h^-j"""
    nat = [0] * S.CELL
    for t, v in enumerate(values):
        nat[S.brp(t, 6)] = v
    h_inv = inv(S.coset_shift(cell_index))
    return [g * pow(h_inv, j, R) % R for j, g in enumerate(_ifft(nat, S.W64))]


def interpolated(cell_indices, cells):
    """cells (64 values each) -> their interpolation polynomials' 64 coefficients each"""
    return [interpolate(i, list(c)) for i, c in zip(cell_indices, cells)]


def column(cell_indices, interp, r, zev=None, zcinv=None):
    """all 128 outputs of column r's decode; interp: interpolated()'s result"""
    if zev is None:
        zev, zcinv = zero_values(cell_indices)
    e = [0] * S.CELLS
    for i, c in zip(cell_indices, interp):
        e[point(i)] = c[r] * zev[point(i)] % R
    nz = _ifft(e, W128)
    shifted = S._fft(scale_by_powers(nz, SHIFT), W128)
    q = _ifft([v * zi % R for v, zi in zip(shifted, zcinv)], W128)
    return scale_by_powers(q, inv(SHIFT))


def recover_columns(cell_indices, cells):
    """route (b): (the 4096 coefficients, the 64 upper halves)"""
    interp = interpolated(cell_indices, cells)
    zev, zcinv = zero_values(cell_indices)
    coeffs, upper = [0] * N, []
    for r in range(S.CELL):
        q = column(cell_indices, interp, r, zev, zcinv)
        for k in range(64):
            coeffs[64 * k + r] = q[k]
        upper.append(q[64:])
    return coeffs, upper


def recover_spec(cell_indices, cells):
    """route (a): the 4096 coefficients by the consensus spec's recover_polynomialcoeff"""
    ext_brp = [0] * S.EXT
    for i, c in zip(cell_indices, cells):
        ext_brp[S.CELL * i: S.CELL * (i + 1)] = list(c)
    ext = [ext_brp[S.brp(k, 13)] for k in range(S.EXT)]
    present = set(cell_indices)
    short = _poly_from_roots([pow(W128, point(i), R) for i in range(S.CELLS) if i not in present])
    zero_poly = [0] * S.EXT
    for k, c in enumerate(short):
        zero_poly[S.CELL * k] = c                                     # the stride of 64
    zero_eval = S._fft(zero_poly, S.W)
    ez = _ifft([a * b % R for a, b in zip(zero_eval, ext)], S.W)      # (E Z)(X) as coefficients
    ez_coset = S._fft(scale_by_powers(ez, SPEC_SHIFT), S.W)
    z_coset = S._fft(scale_by_powers(zero_poly, SPEC_SHIFT), S.W)
    quot = _ifft([a * b % R for a, b in zip(ez_coset, inv_all(z_coset))], S.W)
    return scale_by_powers(quot, inv(SPEC_SHIFT))[:N]


def cells_of(coeffs):
    """the 128 cells of a polynomial as lists of 64 integers"""
    return [S.cell_values(c) for c in S.compute_cells(coeffs)]
