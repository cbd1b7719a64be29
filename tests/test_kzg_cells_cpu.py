"""The host and per-lane pieces of the cell calls (EIP-7594) on the CPU
(build/lb_kzg_cells_harness.so: lb_kzg_transcript.h's cell combiner and deduplication, the phases of
k_fr_coset_ntt4096, k_fr_cell_interp, k_fr_cell_sum and k_fr_cell_quotient and the status fold of
k_kzg_check_cells, compiled for x86) against hashlib and the big-integer helper
tests/kzg_cells_spec.py; lodestar_amd.kzg's restatement of the combiner against the same; the batch
equation itself once through the pure-Python pairing; and a stand-alone program of the harness cases
under the address and undefined-behaviour sanitizers."""
import ctypes
import hashlib
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402

from lodestar_amd import _native as NAT  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402
from oracle import bls_oracle as o  # noqa: E402
from oracle import kzg as OK  # noqa: E402

R = S.R
N = S.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
OKAY, BAD_SCALAR, NOT_IN_GROUP, BAD_ENCODING = NAT.LB_OK, NAT.LB_BAD_SCALAR, NAT.LB_POINT_NOT_IN_GROUP, 1


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_kzg_cells_harness
    lib = ctypes.CDLL(build_kzg_cells_harness(verbose=False))
    c, u = ctypes.c_char_p, ctypes.c_uint32
    lib.c_fr_root8192.argtypes = [c]
    lib.c_kzg_cell_batch_r.argtypes = [u, c, U32, c, c, c, U32, U32]
    lib.c_kzg_cell_batch_r.restype = u
    lib.c_kzg_cell_batch_rs.argtypes = [u, U32, c, U32, c, c, u, c]
    lib.c_fr_coset_ntt4096.argtypes = [c, c]
    lib.c_fr_cell_interp_sum.argtypes = [u, U32, u, c, U32, c, c, c]
    lib.c_fr_cell_interp_sum.restype = u
    lib.c_fr_cell_quotient.argtypes = [c, u, c]
    lib.c_kzg_cell_group_status.argtypes = [I32, u, u, I32, I32, u, u]
    lib.c_kzg_cell_group_status.restype = ctypes.c_int32
    return lib


def _u32(vals):
    a = np.asarray(list(vals) or [0], np.uint32)
    return a, a.ctypes.data_as(U32)


def _le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals) or b"\x00"


def _from_le(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


RND = random.Random(0xCE115)
POLY = [RND.randrange(R) for _ in range(N)]                     # a dense polynomial, by coefficients
CELLS = S.compute_cells(POLY)                                   # computed once, shared, never changed
COMMS = [bytes(RND.randrange(256) for _ in range(48)) for _ in range(4)]   # the transcript takes any 48 bytes
PROOFS = [bytes(RND.randrange(256) for _ in range(48)) for _ in range(8)]


def _hashlib_r(comms, idx, cells, proofs):
    distinct = list(dict.fromkeys(comms))
    data = b"RCKZGCBATCH__V1_" + (4096).to_bytes(8, "big") + (64).to_bytes(8, "big")
    data += len(distinct).to_bytes(8, "big") + len(cells).to_bytes(8, "big") + b"".join(distinct)
    for c, i, cell, p in zip(comms, idx, cells, proofs):
        data += distinct.index(c).to_bytes(8, "big") + i.to_bytes(8, "big") + cell + p
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R


def _c_batch_r(L, comms, idx, cells, proofs):
    n = len(cells)
    out = ctypes.create_string_buffer(32)
    ci, cip = _u32([0xFFFFFFFF] * n)
    first, firstp = _u32([0xFFFFFFFF] * n)
    _, idxp = _u32(idx)
    nd = L.c_kzg_cell_batch_r(n, b"".join(comms) or b"\x00", idxp, b"".join(cells) or b"\x00", b"".join(proofs) or b"\x00",
                              out, cip, firstp)
    return int.from_bytes(out.raw, "big"), nd, ci.tolist()[:n], first.tolist()[:nd]


@pytest.mark.parametrize("n", [0, 1, 3])
def test_cell_batch_r_equals_hashlib(L, n):
    comms, idx, cells, proofs = COMMS[:n], [0, 127, 64][:n], [CELLS[0], CELLS[127], CELLS[64]][:n], PROOFS[:n]
    exp = _hashlib_r(comms, idx, cells, proofs)
    r, nd, ci, first = _c_batch_r(L, comms, idx, cells, proofs)
    assert (r, nd, ci, first) == (exp, n, list(range(n)), list(range(n)))
    assert K.compute_cell_batch_r(comms, idx, cells, proofs) == exp == S.compute_cell_batch_r(comms, idx, cells, proofs)


def test_repeated_commitments_are_deduplicated_in_order_of_first_appearance(L):
    # B A B C A: B sorts after A as bytes or not, the order is the order of appearance
    a, b, c = sorted(COMMS[:3])
    comms, idx = [b, a, b, c, a], [5, 5, 6, 127, 0]
    cells, proofs = [CELLS[i] for i in idx], PROOFS[:5]
    r, nd, ci, first = _c_batch_r(L, comms, idx, cells, proofs)
    assert (nd, ci, first) == (3, [0, 1, 0, 2, 1], [0, 1, 3])
    assert r == _hashlib_r(comms, idx, cells, proofs)
    assert K.compute_cell_batch_r(comms, idx, cells, proofs) == r == S.compute_cell_batch_r(comms, idx, cells, proofs)
    assert S.dedup(comms) == ([b, a, c], ci)


def test_threaded_hashing_equals_single_thread(L):
    sizes = [2, 0, 1, 3, 2]
    off = [0, 2, 2, 3, 6, 8]
    comms = [COMMS[k % 3] for k in range(8)]
    idx = [3 * k for k in range(8)]
    cells = [CELLS[i] for i in idx]
    _, offp = _u32(off)
    _, idxp = _u32(idx)

    def run(threads):
        out = ctypes.create_string_buffer(32 * 5)
        L.c_kzg_cell_batch_rs(5, offp, b"".join(comms), idxp, b"".join(cells), b"".join(PROOFS), threads, out)
        return [int.from_bytes(out.raw[32 * g: 32 * g + 32], "big") for g in range(5)]

    single = run(1)
    assert single == [_hashlib_r(comms[off[g]: off[g + 1]], idx[off[g]: off[g + 1]], cells[off[g]: off[g + 1]],
                                 PROOFS[off[g]: off[g + 1]]) for g in range(5)]
    assert sizes == [off[g + 1] - off[g] for g in range(5)]
    for threads in (2, 5, 16):   # fewer, as many and more threads than groups
        assert run(threads) == single, threads


def test_helper_identities(L):
    """the helper's own cells: 0 .. 63 are the blob; values are Horner evaluations at the coset points"""
    blob = S.coefficients_to_blob(POLY)
    assert b"".join(CELLS[:64]) == blob
    assert S.blob_coefficients(blob) == POLY
    assert S.blob_values(blob)[1] == S.horner(POLY, OK.roots_brp(N)[1])
    for i in (0, 63, 64, 127):
        vals = S.cell_values(CELLS[i])
        for t in (0, 1, 63):
            assert vals[t] == S.horner(POLY, S.coset_point(i, t)), (i, t)
        assert K.coset_shift(i) == S.coset_shift(i)
    out = ctypes.create_string_buffer(32)
    L.c_fr_root8192(out)
    assert int.from_bytes(out.raw, "little") == S.W == K.ROOT_OF_UNITY_EXT
    assert (K.BYTES_PER_CELL, K.CELLS_PER_EXT_BLOB, K.FIELD_ELEMENTS_PER_EXT_BLOB) == (2048, 128, 8192)


@pytest.mark.parametrize("poly", ["random", "zero", "top"])
def test_coset_transform_phases(L, poly):
    coeffs = {"random": POLY, "zero": [0] * N, "top": [0] * (N - 1) + [1]}[poly]
    exp = CELLS if poly == "random" else S.compute_cells(coeffs)
    out = ctypes.create_string_buffer(32 * N)
    L.c_fr_coset_ntt4096(_le(coeffs), out)
    assert out.raw == b"".join(exp[64:])


def _interp(L, off, idx, cells, weights):
    ng, nc = len(off) - 1, len(cells)
    coeffs = ctypes.create_string_buffer(max(32 * 64 * nc, 1))
    sums = ctypes.create_string_buffer(max(32 * 64 * ng, 1))
    _, offp = _u32(off)
    _, idxp = _u32(idx)
    bad = L.c_fr_cell_interp_sum(ng, offp, nc, b"".join(cells) or b"\x00", idxp, _le(weights), coeffs, sums)
    return bad, _from_le(coeffs.raw, 64 * nc), _from_le(sums.raw, 64 * ng)


def test_cell_interpolation_lanes(L):
    """unit weights: the descaled coefficients reproduce all 64 values of the cell by Horner, and
    equal the helper's direct inverse DFT; a constant cell has one coefficient"""
    idx = [0, 1, 64, 127, 9]
    cells = [CELLS[i] for i in idx[:4]] + [S.values_to_blob([77] * 64)]
    bad, coeffs, _ = _interp(L, [0, 5], idx, cells, [1] * 5)
    assert bad == 0
    for c, i in enumerate(idx):
        got = coeffs[64 * c: 64 * c + 64]
        vals = S.cell_values(cells[c])
        assert [S.horner(got, S.coset_point(i, t)) for t in range(64)] == vals, i
        assert got == S.interpolate(i, vals), i
    assert coeffs[64 * 4: 64 * 5] == [77] + [0] * 63
    over = S.values_to_blob([R] + [0] * 63)
    assert _interp(L, [0, 1], [0], [over], [1])[0] == 1       # an element equal to r is reported


def test_cell_group_sums(L):
    """groups of 0, 1 and 65 cells with distinct weights: the negated sums of the weighted coefficients"""
    rnd = random.Random(65)
    off = [0, 0, 1, 66]
    idx = [rnd.randrange(128) for _ in range(66)]
    cells = [CELLS[i] for i in idx]
    weights = [rnd.randrange(1, R) for _ in range(66)]
    _, coeffs, sums = _interp(L, off, idx, cells, weights)
    per_cell = {}
    for g in range(3):
        exp = [0] * 64
        for k in range(off[g], off[g + 1]):
            if idx[k] not in per_cell:
                per_cell[idx[k]] = S.interpolate(idx[k], S.cell_values(cells[k]))
            mine = [weights[k] * c % R for c in per_cell[idx[k]]]
            assert coeffs[64 * k: 64 * k + 64] == mine, k
            exp = [(a + b) % R for a, b in zip(exp, mine)]
        assert sums[64 * g: 64 * g + 64] == [(-v) % R for v in exp], g
    assert sums[:64] == [0] * 64


@pytest.mark.parametrize("cell", [0, 127])
def test_cell_quotient_lanes(L, cell):
    low = POLY[:64] + [0] * (N - 64)        # degree 63: the quotient is zero
    for coeffs in (POLY, low):
        q = ctypes.create_string_buffer(32 * N)
        L.c_fr_cell_quotient(_le(coeffs), cell, q)
        exp_q, exp_i = S.cell_quotient(coeffs, cell)
        assert _from_le(q.raw, N) == exp_q + [0] * 64
        assert exp_i == S.interpolate(cell, [S.horner(coeffs, S.coset_point(cell, t)) for t in range(64)])
    assert exp_q == [0] * (N - 64)


def _fold(L, doff, off, g, dst, cst, pst):
    d = np.asarray(dst + [OKAY], np.int32)
    c = np.asarray(cst + [OKAY], np.int32)
    p = np.asarray(pst + [OKAY], np.int32)
    return L.c_kzg_cell_group_status(d.ctypes.data_as(I32), doff[g], doff[g + 1], c.ctypes.data_as(I32), p.ctypes.data_as(I32),
                                     off[g], off[g + 1])


def test_status_fold(L):
    """groups of 0, 1 and 3 cells (offsets 0,0,1,4; the last with 2 distinct commitments): every error
    kind at every position; any commitment before any cell before any proof; lowest position within a kind"""
    off, doff = [0, 0, 1, 4], [0, 0, 1, 3]
    clean_d, clean_c = [OKAY] * 3, [OKAY] * 4
    for g in range(3):
        assert _fold(L, doff, off, g, clean_d, clean_c, clean_c) == OKAY
    for d in range(3):
        for code in (NOT_IN_GROUP, BAD_ENCODING):
            dst = list(clean_d)
            dst[d] = code
            for g in range(3):
                assert _fold(L, doff, off, g, dst, clean_c, clean_c) == (code if g == (1 if d == 0 else 2) else OKAY)
    for j in range(4):
        mine = 1 if j == 0 else 2
        cst = list(clean_c)
        cst[j] = BAD_SCALAR
        for g in range(3):
            assert _fold(L, doff, off, g, clean_d, cst, clean_c) == (BAD_SCALAR if g == mine else OKAY)
        for code in (NOT_IN_GROUP, BAD_ENCODING):
            pst = list(clean_c)
            pst[j] = code
            for g in range(3):
                assert _fold(L, doff, off, g, clean_d, clean_c, pst) == (code if g == mine else OKAY)
    # precedence in the group of three: the last proof, then an earlier proof, then the last cell,
    # then an earlier cell (stored with any code: it reads as LB_BAD_SCALAR), then the commitments
    dst, cst, pst = list(clean_d), list(clean_c), list(clean_c)
    pst[3] = NOT_IN_GROUP
    assert _fold(L, doff, off, 2, dst, cst, pst) == NOT_IN_GROUP
    pst[1] = BAD_ENCODING
    assert _fold(L, doff, off, 2, dst, cst, pst) == BAD_ENCODING
    cst[3] = BAD_SCALAR
    assert _fold(L, doff, off, 2, dst, cst, pst) == BAD_SCALAR
    cst[3], cst[2] = OKAY, 5
    assert _fold(L, doff, off, 2, dst, cst, pst) == BAD_SCALAR
    dst[2] = NOT_IN_GROUP
    assert _fold(L, doff, off, 2, dst, cst, pst) == NOT_IN_GROUP
    dst[1] = BAD_ENCODING
    assert _fold(L, doff, off, 2, dst, cst, pst) == BAD_ENCODING
    assert _fold(L, doff, off, 1, dst, cst, pst) == OKAY and _fold(L, doff, off, 0, dst, cst, pst) == OKAY


def test_batch_equation_through_the_python_pairing():
    """p of degree 67 with its commitment and the proofs of cells 3 and 100 by the oracle's sparse
    commitments (4-term quotients): the helper's equation accepts them, rejects one changed cell
    element and rejects the two cell indices swapped -- three pairing products, the pin of the equation"""
    g1, g2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
    rnd = random.Random(67)
    coeffs = [rnd.randrange(R) for _ in range(68)]
    commitment = o.g1_compress(OK.commit_monomials(g1, dict(enumerate(coeffs))))
    all_cells = S.compute_cells(coeffs)
    idx, cells, proofs = [3, 100], [], []
    for i in idx:
        q, rem = S.cell_quotient(coeffs, i)
        assert len(q) == 4 and rem == S.interpolate(i, S.cell_values(all_cells[i]))
        cells.append(all_cells[i])
        proofs.append(o.g1_compress(OK.commit_monomials(g1, dict(enumerate(q)))))
    comms = [commitment, commitment]
    assert S._lincomb(g1[:4], q) == proofs[1]            # the helper's shared-doubling sum is the oracle's
    assert S.batch_equation(comms, idx, cells, proofs, g1, g2) is True
    vals = S.cell_values(cells[1])
    vals[5] = (vals[5] + 1) % R
    assert S.batch_equation(comms, idx, [cells[0], S.values_to_blob(vals)], proofs, g1, g2) is False
    assert S.batch_equation(comms, idx[::-1], cells, proofs, g1, g2) is False
    assert S.batch_equation([], [], [], [], g1, g2) is True


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cell_pieces_under_sanitizers(tmp_path):
    """tests/native/kzg_cells_check.cpp: the harness cases in a program of its own, built with
    -fsanitize=address,undefined and run directly (-g1: line tables are all a report needs, and full
    debug information of the inlined field code triples the compile time)"""
    exe = tmp_path / "kzg_cells_check"
    subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "harness"),
                    os.path.join(ROOT, "tests", "native", "kzg_cells_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kzg_cells_check: failures 0" in out.stdout
