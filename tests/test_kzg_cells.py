"""The cell calls (EIP-7594) on the GPU: lb_kzg_compute_cells, lb_kzg_compute_cell_proofs and
lb_kzg_verify_cell_proof_batch (C ABI), and the Python surface over them (Kzg.compute_cells,
compute_cell_kzg_proofs, verify_cell_kzg_proof_batch(_many) and the ckzg aliases).

Expected values never come from the calls under test: cells from tests/kzg_cells_spec.py's Python
transform, commitments and proofs from its Python long division committed through the host-mode
group call (lb_g1_lincomb over the resident setup), verdicts by construction (proofs that are right
accept; one changed input rejects).  The equation itself is pinned on the CPU through the
pure-Python pairing (tests/test_kzg_cells_cpu.py).  Two blobs, a dense one and one of degree 70
(cheap proofs), in groups of 0, 1, 3, 0 and 66 cells, built once per module."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
from test_kzg_batch import _off_subgroup_g1  # noqa: E402

from lodestar_amd import _native as N  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402
from oracle import bls_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

R = o.R
INF = bytes([0xC0]) + bytes(47)
U8, U32, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
SIZES = [0, 1, 3, 0, 66]
OFFSETS = [0, 0, 1, 4, 4, 70]
DENSE, LOW = 0, 1
_rnd = random.Random(0x7594)
COEFFS = [[_rnd.randrange(R) for _ in range(S.N)], [_rnd.randrange(R) for _ in range(71)]]
BLOBS = [S.coefficients_to_blob(c) for c in COEFFS]
CELLS = [S.compute_cells(c) for c in COEFFS]
# (blob, cell index) per position.  The 66-cell group crosses the 64-lane stride, mixes both blobs (two
# distinct commitments), holds cell indices 0, 63, 64 and 127 and repeats one (commitment, cell) pair.
_DENSE_IN_BIG = [0, 63, 64, 127, 5, 70]
_LOW_IN_BIG = [i for i in range(2, 128, 2) if i not in (64,)][:58] + [127]
PAIRS = ([(DENSE, 0)] + [(LOW, 63), (DENSE, 64), (LOW, 127)]
         + [(DENSE, i) for i in _DENSE_IN_BIG[:3]] + [(LOW, i) for i in _LOW_IN_BIG] + [(DENSE, i) for i in _DENSE_IN_BIG[3:]]
         + [(LOW, _LOW_IN_BIG[7])])
assert len(PAIRS) == 70 and len(set(PAIRS[4:])) == 65


@pytest.fixture(scope="module")
def host(engine):
    return K.Kzg(engine)


@pytest.fixture(scope="module")
def fx(host):
    """commitments and proofs by the helper's coefficients and long division through host-mode
    lb_g1_lincomb; the flat per-cell arrays of the five groups"""
    comms = [host.g1_lincomb(c) for c in COEFFS]
    proof_of = {}
    for pair in sorted(set(PAIRS) | {(DENSE, i) for i in (0, 63, 64, 127)}):
        q, _ = S.cell_quotient(COEFFS[pair[0]], pair[1])
        proof_of[pair] = host.g1_lincomb(q)
    return {"comms": comms, "proof_of": proof_of,
            "c": [comms[b] for b, _ in PAIRS], "i": [i for _, i in PAIRS],
            "cells": [CELLS[b][i] for b, i in PAIRS], "p": [proof_of[pair] for pair in PAIRS]}


def c_verify(engine_h, comms, idx, cells, proofs, offsets=OFFSETS):
    """the C call over flat lists; returns (rc, out_ok as a list)"""
    lib = N.load()
    n = len(offsets) - 1
    cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
    ce = np.frombuffer(b"".join(cells) or b"\x00", np.uint8)
    pf = np.frombuffer(b"".join(proofs) or b"\x00", np.uint8)
    ci = np.asarray(list(idx) or [0], np.uint32)
    off = np.asarray(offsets, np.uint32)
    out = np.full(max(n, 1), -99, np.int32)
    rc = lib.lb_kzg_verify_cell_proof_batch(engine_h, n, off.ctypes.data_as(U32), cm.ctypes.data_as(U8), ci.ctypes.data_as(U32),
                                            ce.ctypes.data_as(U8), pf.ctypes.data_as(U8), out.ctypes.data_as(I32))
    return rc, out.tolist()[:n]


def c_cells(engine_h, blobs):
    lib = N.load()
    n = len(blobs)
    bl = np.frombuffer(b"".join(blobs), np.uint8)
    out = np.full(n * 128 * 2048, 0xEE, np.uint8)
    st = np.full(n, -99, np.int32)
    rc = lib.lb_kzg_compute_cells(engine_h, n, bl.ctypes.data_as(U8), out.ctypes.data_as(U8), st.ctypes.data_as(I32))
    raw = out.tobytes()
    return rc, [[raw[(128 * b + i) * 2048: (128 * b + i + 1) * 2048] for i in range(128)] for b in range(n)], st.tolist()


def sub(lst, j, v):
    return lst[:j] + [v] + lst[j + 1:]


def test_compute_cells_equal_the_python_transform(host):
    h = host.engine.h
    rc, cells, st = c_cells(h, [BLOBS[DENSE]])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert cells[0] == CELLS[DENSE]
    assert b"".join(cells[0][:64]) == BLOBS[DENSE]
    rc, cells, st = c_cells(h, [bytes(K.BYTES_PER_BLOB)])
    assert (rc, st) == (N.LB_OK, [N.LB_OK]) and cells[0] == [bytes(2048)] * 128
    # two blobs in one call; then one element equal to r in the first of two
    rc, cells, st = c_cells(h, [BLOBS[LOW], BLOBS[DENSE]])
    assert (rc, st) == (N.LB_OK, [N.LB_OK] * 2) and cells == [CELLS[LOW], CELLS[DENSE]]
    elem_r = BLOBS[LOW][:32 * 70] + R.to_bytes(32, "big") + BLOBS[LOW][32 * 71:]
    rc, cells, st = c_cells(h, [elem_r, BLOBS[LOW]])
    assert (rc, st) == (N.LB_OK, [N.LB_BAD_SCALAR, N.LB_OK])
    assert cells[0] == [bytes(2048)] * 128 and cells[1] == CELLS[LOW]
    assert host.compute_cells(BLOBS[LOW]) == CELLS[LOW] == host.computeCells(BLOBS[LOW])
    with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
        host.compute_cells(elem_r)
    lib = N.load()
    assert lib.lb_kzg_compute_cells(h, 0, None, None, None) == N.LB_OK
    assert lib.lb_kzg_compute_cells(h, 1025, None, None, None) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_compute_cells(h, 1, None, None, None) == N.LB_ERR_ARGUMENT


def test_cell_proofs_equal_the_python_quotient(host, fx):
    idx = [0, 63, 64, 127]
    assert host.compute_cell_kzg_proofs(BLOBS[DENSE], idx) == [fx["proof_of"][(DENSE, i)] for i in idx]
    assert host.compute_cell_kzg_proofs(BLOBS[LOW], [63, 63]) == [fx["proof_of"][(LOW, 63)]] * 2
    assert host.compute_cell_kzg_proofs(BLOBS[LOW], []) == []
    with pytest.raises(K.KzgError):
        host.compute_cell_kzg_proofs(BLOBS[LOW], [128])
    lib = N.load()
    bl = np.frombuffer(BLOBS[LOW], np.uint8)
    ci = np.asarray([128], np.uint32)
    out, st = np.zeros(48, np.uint8), np.zeros(1, np.int32)
    assert lib.lb_kzg_compute_cell_proofs(host.engine.h, bl.ctypes.data_as(U8), 1, ci.ctypes.data_as(U32), out.ctypes.data_as(U8),
                                          st.ctypes.data_as(I32)) == N.LB_ERR_ARGUMENT
    elem_r = R.to_bytes(32, "big") + BLOBS[LOW][32:]
    with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
        host.compute_cell_kzg_proofs(elem_r, [0])


def test_every_cell_of_a_constant_blob_has_the_infinity_proof(host):
    blob = S.values_to_blob([9] * S.N)
    assert host.compute_cell_kzg_proofs(blob, list(range(128))) == [INF] * 128


def test_all_groups_accepted(host, fx, monkeypatch):
    h = host.engine.h
    assert c_verify(h, fx["c"], fx["i"], fx["cells"], fx["p"]) == (N.LB_OK, [1] * 5)
    assert N.load().lb_kzg_batch_hash_ns(h) > 0
    monkeypatch.setenv("LB_KZG_HASH_THREADS", "1")      # one hashing thread: the same verdicts
    assert c_verify(h, fx["c"], fx["i"], fx["cells"], fx["p"]) == (N.LB_OK, [1] * 5)
    # a constant polynomial: infinity proofs, and the infinity commitment for the zero polynomial
    const = S.compute_cells([9])
    c9 = host.g1_lincomb([9])
    assert c_verify(h, [c9, c9, INF], [0, 127, 64], [const[0], const[127], bytes(2048)], [INF] * 3, [0, 2, 3]) == (N.LB_OK, [1, 1])
    assert c_verify(h, [c9], [5], [S.values_to_blob([10] * 64)], [INF], [0, 1]) == (N.LB_OK, [0])


def test_exactly_one_point_at_infinity_rejects(host):
    """one group of one cell (its combiner power is r^0 = 1, so the points can be chosen): the cell is
    the constant v, the proof pi = [s] G1 and the commitment C = [v - h^64 s] G1, which makes
    RL = C + [h^64] pi - [v] G1 the point at infinity under a finite LL = pi: e(pi, [tau^64] G2) alone
    is not 1.  The converse (LL at infinity, RL not) is the constant cell with the wrong commitment of
    test_all_groups_accepted."""
    h = host.engine.h
    v, s, idx = 10, 0x5EED, 5
    h64 = pow(K.coset_shift(idx), 64, R)
    pi = o.g1_compress(o.g1_mul(o.G1, s))
    comm = o.g1_compress(o.g1_mul(o.G1, (v - h64 * s) % R))
    cell = S.values_to_blob([v] * 64)
    assert c_verify(h, [comm], [idx], [cell], [pi], [0, 1]) == (N.LB_OK, [0])
    # the same cell under its own commitment and proof accepts: both points at infinity
    assert c_verify(h, [o.g1_compress(o.g1_mul(o.G1, v))], [idx], [cell], [INF], [0, 1]) == (N.LB_OK, [1])


def test_rejections_stay_local(host, fx):
    h = host.engine.h
    c, i, cells, p = fx["c"], fx["i"], fx["cells"], fx["p"]
    # one cell element + 1, beyond the 64th cell of the big group
    k = 4 + 65
    vals = S.cell_values(cells[k])
    vals[17] = (vals[17] + 1) % R
    assert c_verify(h, c, i, sub(cells, k, S.values_to_blob(vals)), p) == (N.LB_OK, [1, 1, 1, 1, 0])
    # a proof swapped with its neighbour's
    assert c_verify(h, c, i, cells, sub(sub(p, 1, p[2]), 2, p[1])) == (N.LB_OK, [1, 1, 0, 1, 1])
    # a cell index off by one
    assert c_verify(h, c, sub(i, 0, 1), cells, p) == (N.LB_OK, [1, 0, 1, 1, 1])
    # a commitment replaced by the other blob's
    other = fx["comms"][LOW] if PAIRS[10][0] == DENSE else fx["comms"][DENSE]
    assert c_verify(h, sub(c, 10, other), i, cells, p) == (N.LB_OK, [1, 1, 1, 1, 0])


def test_errors_and_their_precedence(host, fx):
    h = host.engine.h
    c, i, cells, p = fx["c"], fx["i"], fx["cells"], fx["p"]
    off_g1 = o.g1_compress(_off_subgroup_g1())
    flagless = bytearray(fx["comms"][DENSE])
    flagless[0] &= 0x7F                                   # compression flag cleared
    flagless = bytes(flagless)
    lib = N.load()
    one = (ctypes.c_uint8 * 32)(1)
    out48 = (ctypes.c_uint8 * 48)()
    bad_code = lib.lb_g1_lincomb(h, 1, ctypes.cast((ctypes.c_uint8 * 48).from_buffer_copy(flagless), U8),
                                 ctypes.cast(one, U8), ctypes.cast(out48, U8))   # the decode code of the existing call
    assert bad_code not in (N.LB_OK, N.LB_POINT_NOT_IN_GROUP, N.LB_BAD_SCALAR)
    elem_r = cells[2][:2016] + R.to_bytes(32, "big")
    assert c_verify(h, c, i, sub(cells, 2, elem_r), p) == (N.LB_OK, [1, 1, -N.LB_BAD_SCALAR, 1, 1])
    assert c_verify(h, c, i, cells, sub(p, 0, off_g1)) == (N.LB_OK, [1, -N.LB_POINT_NOT_IN_GROUP, 1, 1, 1])
    assert c_verify(h, sub(c, 69, off_g1), i, cells, p) == (N.LB_OK, [1, 1, 1, 1, -N.LB_POINT_NOT_IN_GROUP])
    assert c_verify(h, sub(c, 3, flagless), i, cells, p) == (N.LB_OK, [1, 1, -bad_code, 1, 1])
    assert c_verify(h, c, i, cells, sub(p, 40, flagless)) == (N.LB_OK, [1, 1, 1, 1, -bad_code])

    def group3(cc, ce, pp):
        rc, got = c_verify(h, cc, i, ce, pp)
        assert rc == N.LB_OK and got[:2] + got[3:] == [1] * 4
        return got[2]

    # two errors in the group of three (positions 1, 2, 3): a cell before an EARLIER proof,
    # a LATER commitment before both, and the lower position within a kind
    assert group3(c, sub(cells, 3, elem_r[-32:] + cells[3][32:]), sub(p, 1, off_g1)) == -N.LB_BAD_SCALAR
    assert group3(sub(c, 3, flagless), sub(cells, 2, elem_r), sub(p, 1, off_g1)) == -bad_code
    assert group3(c, cells, sub(sub(p, 3, flagless), 2, off_g1)) == -N.LB_POINT_NOT_IN_GROUP
    assert group3(sub(sub(c, 3, flagless), 1, off_g1), cells, p) == -N.LB_POINT_NOT_IN_GROUP


def test_argument_errors(host, fx):
    from lodestar_amd.engine import Engine
    h = host.engine.h
    one = ([fx["c"][0]], [fx["i"][0]], [fx["cells"][0]], [fx["p"][0]])
    assert c_verify(h, *one, [0, 1]) == (N.LB_OK, [1])
    assert c_verify(h, one[0], [128], one[2], one[3], [0, 1]) == (N.LB_ERR_ARGUMENT, [-99])
    assert c_verify(h, *one, [1, 1])[0] == N.LB_ERR_ARGUMENT
    assert c_verify(h, *one, [0, 1, 0])[0] == N.LB_ERR_ARGUMENT            # decreasing offsets
    assert c_verify(h, *one, [0] * 1026)[0] == N.LB_ERR_ARGUMENT
    assert c_verify(h, *one, [0, 16385])[0] == N.LB_ERR_ARGUMENT           # rejected before any cell is read
    lib = N.load()
    assert lib.lb_kzg_verify_cell_proof_batch(h, 0, None, None, None, None, None, None) == N.LB_OK
    off = np.asarray([0, 1], np.uint32)
    assert lib.lb_kzg_verify_cell_proof_batch(h, 1, off.ctypes.data_as(U32), None, None, None, None,
                                              np.zeros(1, np.int32).ctypes.data_as(I32)) == N.LB_ERR_ARGUMENT
    # a setup loaded with two G2 points: everything but the cell verification works
    g1, g2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
    with Engine(0) as fresh:
        assert c_verify(fresh.h, *one, [0, 1])[0] == N.LB_ERR_ARGUMENT     # no setup at all
        g1b, g2b = np.frombuffer(b"".join(g1), np.uint8), np.frombuffer(b"".join(g2[:2]), np.uint8)
        st = np.zeros(len(g1), np.int32)
        assert lib.lb_kzg_load_setup(fresh.h, g1b.ctypes.data_as(U8), len(g1), g2b.ctypes.data_as(U8), 2,
                                     st.ctypes.data_as(I32)) == N.LB_OK
        assert c_verify(fresh.h, *one, [0, 1]) == (N.LB_ERR_ARGUMENT, [-99])
        z = 12345
        proof, y = host.compute_kzg_proof_coefficients(COEFFS[LOW], z)
        ok = ctypes.c_int32(-99)
        le = lambda v: ctypes.cast((ctypes.c_uint8 * 32).from_buffer_copy(int(v).to_bytes(32, "little")), U8)   # noqa: E731
        b48 = lambda b: ctypes.cast((ctypes.c_uint8 * 48).from_buffer_copy(b), U8)   # noqa: E731
        assert lib.lb_kzg_verify_proof(fresh.h, b48(fx["comms"][LOW]), le(z), le(y), b48(proof), ctypes.byref(ok)) == N.LB_OK
        assert ok.value == 1
        rc, cells, st1 = c_cells(fresh.h, [BLOBS[LOW]])
        assert (rc, st1) == (N.LB_OK, [N.LB_OK]) and cells[0] == CELLS[LOW]


def test_python_surface(engine, host, fx):
    c, i, cells, p = fx["c"], fx["i"], fx["cells"], fx["p"]
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r = R.to_bytes(32, "big") + cells[1][32:]
    g = lambda lo, hi: (c[lo:hi], i[lo:hi], cells[lo:hi], p[lo:hi])   # noqa: E731
    groups = [g(1, 4), (c[1:4], i[1:4], cells[1:4], [p[2], p[1], p[3]]), (c[1:4], i[1:4], [elem_r] + cells[2:4], p[1:4]),
              (c[1:4], i[1:4], cells[1:4], [p[1], off_g1, p[3]]), ([], [], [], []), g(4, 70)]
    for kz in (host, K.Kzg(engine, field="device")):     # always the device call, whatever `field` is
        got = kz.verify_cell_kzg_proof_batch_many(groups)
        assert got[0] is True and got[1] is False and got[4] is True and got[5] is True
        assert isinstance(got[2], K.KzgError) and "BLST_BAD_SCALAR" in str(got[2])
        assert isinstance(got[3], K.KzgError) and "BLST_POINT_NOT_IN_GROUP" in str(got[3])
        assert kz.verifyCellKzgProofBatch(*groups[0]) is True
        assert kz.verifyCellKzgProofBatch(*groups[1]) is False
        assert kz.verify_cell_kzg_proof_batch([], [], [], []) is True
        with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
            kz.verifyCellKzgProofBatch(*groups[2])
    assert host.verifyCellKzgProofBatchMany([]) == []
    # malformed input raises before anything is sent
    with pytest.raises(K.KzgError):
        host.verifyCellKzgProofBatch(c[1:4], i[1:4], cells[1:4], p[1:3])
    with pytest.raises(K.KzgError):
        host.verifyCellKzgProofBatch(c[1:2], [128], cells[1:2], p[1:2])
    with pytest.raises(K.KzgError):
        host.verifyCellKzgProofBatch(c[1:2], i[1:2], [cells[1][:-1]], p[1:2])
    with pytest.raises(K.KzgError):
        host.verifyCellKzgProofBatch([c[1][:47]], i[1:2], cells[1:2], p[1:2])


def write_js_fixture(path, host, fx):
    """the bytes tests/js/test_kzg_cells.js checks the JS surface against (tests/test_js_kzg_cells.py)"""
    hx = lambda bs: [b.hex() for b in bs]   # noqa: E731
    with open(path, "w") as f:
        json.dump({"blob": BLOBS[LOW].hex(), "cells": hx(CELLS[LOW]),
                   "commitments": hx(fx["c"][1:4]), "cellIndices": fx["i"][1:4], "groupCells": hx(fx["cells"][1:4]),
                   "proofs": hx(fx["p"][1:4])}, f)
