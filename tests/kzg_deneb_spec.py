"""Big-integer restatement of the per-blob (Deneb) KZG proof form, for the tests (a helper, not
collected).  Independent of lodestar_amd/kzg.py: it builds on oracle/kzg.py (the barycentric
evaluation, the pairing check, sparse commitments) and oracle/bls_oracle.py alone.

    z_i = hash_to_bls_field(FS_DOMAIN || 4096 as 16 bytes BE || blob_i || C_i)
    y_i = p_i(z_i)
    r   = hash_to_bls_field(RC_DOMAIN || 4096 as 8 bytes BE || n as 8 bytes BE ||
                            for each i: C_i || z_i (32 BE) || y_i (32 BE) || proof_i)
    T   = sum r^i C_i - [sum r^i y_i] G1 + sum [r^i z_i] proof_i,    P = sum r^i proof_i
    accept iff e(T, -G2) e(P, [tau] G2) == 1;  n = 0 accepts

Errors are not verdicts: a blob element >= r, a commitment or proof that fails to decode or lies
outside G1.  The lowest blob index with any error wins; within a blob the order is commitment, blob
element, proof."""
import hashlib

from oracle import bls_oracle as o
from oracle import kzg as OK

R = o.R
N = 4096
FS_DOMAIN = b"FSBLOBVERIFY_V1_"
RC_DOMAIN = b"RCKZGBATCH___V1_"
G1_GENERATOR48 = o.g1_compress(o.G1)
INF48 = bytes([0xC0]) + bytes(47)
ROOTS_BRP = OK.roots_brp(N)


def hash_to_bls_field(data):
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R


def compute_challenge(blob, commitment48):
    assert len(blob) == 32 * N and len(commitment48) == 48
    return hash_to_bls_field(FS_DOMAIN + N.to_bytes(16, "big") + bytes(blob) + bytes(commitment48))


def compute_batch_r(commitments, zs, ys, proofs):
    data = RC_DOMAIN + N.to_bytes(8, "big") + len(commitments).to_bytes(8, "big")
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        data += bytes(c) + z.to_bytes(32, "big") + y.to_bytes(32, "big") + bytes(p)
    return hash_to_bls_field(data)


def blob_values(blob):
    """the blob's field elements, or None if one is >= r"""
    vals = [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(N)]
    return None if any(v >= R for v in vals) else vals


def evaluate_blob(blob, z):
    return OK.evaluate_polynomial_in_evaluation_form(blob_values(blob), z, ROOTS_BRP)


def batch_terms(commitments, zs, ys, proofs):
    """the batch equation as two linear combinations: (points, scalars) of T and of P"""
    n = len(commitments)
    r = compute_batch_r(commitments, zs, ys, proofs)
    pw = [pow(r, i, R) for i in range(n)]
    t_points = list(commitments) + list(proofs) + [G1_GENERATOR48]
    t_scalars = pw + [pw[i] * zs[i] % R for i in range(n)] + [-sum(pw[i] * ys[i] for i in range(n)) % R]
    return (t_points, t_scalars), (list(proofs), pw)


def _lincomb(points, scalars):
    acc = None
    for p48, s in zip(points, scalars):
        acc = o.g1_add(acc, o.g1_mul(o.g1_decompress(p48), s))
    return o.g1_compress(acc)


def batch_equation(commitments, zs, ys, proofs, setup_g2, lincomb=_lincomb, pairing_check=None):
    """e(T, -G2) e(P, [tau] G2) == 1.  By default everything is pure Python; `lincomb(points48,
    scalars) -> 48 bytes` and `pairing_check(T48, P48) -> bool` let a test run the same equation
    through other group code."""
    if not commitments:
        return True
    (tp, ts), (pp, ps) = batch_terms(commitments, zs, ys, proofs)
    t48, p48 = lincomb(tp, ts), lincomb(pp, ps)
    if pairing_check is not None:
        return pairing_check(t48, p48)
    # verify_kzg_proof_impl at z = y = 0: e(T - 0, -G2) e(P, [tau] G2 - 0)
    return bool(OK.verify_kzg_proof_impl(t48, 0, 0, p48, setup_g2))


def low_degree_blob(coeffs):
    """the blob of p(X) = sum coeffs[k] X^k: its evaluations at the bit-reversed roots of unity"""
    vals = []
    for w in ROOTS_BRP:
        y = 0
        for c in reversed(coeffs):
            y = (y * w + c) % R
        vals.append(y)
    return b"".join(v.to_bytes(32, "big") for v in vals)


def synthetic_division(coeffs, z):
    """(y, q) with p(X) - y = (X - z) q(X); q has len(coeffs) - 1 coefficients"""
    q = [0] * (len(coeffs) - 1)
    acc = 0
    for k in range(len(coeffs) - 1, 0, -1):
        acc = (acc * z + coeffs[k]) % R
        q[k - 1] = acc
    return (acc * z + coeffs[0]) % R, q


def low_degree_proof(setup_g1, coeffs):
    """(blob, commitment, z, y, proof) for a short coefficient list, by the oracle alone"""
    blob = low_degree_blob(coeffs)
    commitment = o.g1_compress(OK.commit_monomials(setup_g1, dict(enumerate(coeffs))))
    z = compute_challenge(blob, commitment)
    y, q = synthetic_division(coeffs, z)
    proof = o.g1_compress(OK.commit_monomials(setup_g1, dict(enumerate(q))))
    return blob, commitment, z, y, proof
