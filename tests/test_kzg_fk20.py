"""lb_kzg_compute_cells_and_proofs (c-kzg computeCellsAndKzgProofs by FK20) on the GPU, and the
Python surface over it (Kzg.compute_cells_and_kzg_proofs(_many) and the ckzg aliases).

Expected values never come from the call under test: cells from tests/kzg_cells_spec.py's Python
transform; proofs from its Python long division committed through the host-mode group call
(lb_g1_lincomb over the resident setup), and for the dense blob also from the direct per-cell route
lb_kzg_compute_cell_proofs; acceptance by the existing cell verifier.  The dense blob and the degree-70 blob are those of tests/test_kzg_cells.py;
their references are built once per module."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
from test_kzg_cells import BLOBS, CELLS, COEFFS, DENSE, LOW  # noqa: E402

from lodestar_amd import _native as N  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402

pytestmark = pytest.mark.gpu

R = S.R
INF = bytes([0xC0]) + bytes(47)
U8, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
ALL = list(range(128))
_rnd = random.Random(0xF1220)
SETUP_G1, SETUP_G2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())


def c_call(engine_h, blobs):
    """the C call; returns (rc, per blob its 128 cells, per blob its 128 proofs, statuses)"""
    lib = N.load()
    n = len(blobs)
    bl = np.frombuffer(b"".join(blobs), np.uint8)
    cells = np.full(n * 128 * 2048, 0xEE, np.uint8)
    proofs = np.full(n * 128 * 48, 0xEE, np.uint8)
    st = np.full(n, -99, np.int32)
    rc = lib.lb_kzg_compute_cells_and_proofs(engine_h, n, bl.ctypes.data_as(U8), cells.ctypes.data_as(U8), proofs.ctypes.data_as(U8),
                                             st.ctypes.data_as(I32))
    craw, praw = cells.tobytes(), proofs.tobytes()
    return (rc, [[craw[(128 * b + i) * 2048: (128 * b + i + 1) * 2048] for i in ALL] for b in range(n)],
            [[praw[(128 * b + i) * 48: (128 * b + i + 1) * 48] for i in ALL] for b in range(n)], st.tolist())


def commit(host, quotient):
    """commit(quotient) over the resident setup, as short as the quotient is"""
    q = list(quotient)
    while q and q[-1] == 0:
        q.pop()
    return host.g1_lincomb(q) if q else INF


@pytest.fixture(scope="module")
def host(engine):
    return K.Kzg(engine)


@pytest.fixture(scope="module")
def ref(host):
    """the references of the dense and the degree-70 blob, computed once: proofs by long division and
    host-mode lb_g1_lincomb, by the direct per-cell route, and this call's own single-blob outputs"""
    by_division = [host.g1_lincomb(S.cell_quotient(COEFFS[DENSE], i)[0]) for i in ALL]
    direct = host.compute_cell_kzg_proofs(BLOBS[DENSE], ALL)
    low = host.g1_lincomb(S.cell_quotient(COEFFS[LOW], 0)[0])         # degree 70: Q = a[64 .. 70], the same for every cell
    single = {}
    for b in (DENSE, LOW):
        rc, cells, proofs, st = c_call(host.engine.h, [BLOBS[b]])
        assert (rc, st) == (N.LB_OK, [N.LB_OK])
        single[b] = (cells[0], proofs[0])
    return {"by_division": by_division, "direct": direct, "low": low, "single": single}


def test_dense_blob_cells_and_all_128_proofs(ref):
    cells, proofs = ref["single"][DENSE]
    assert cells == CELLS[DENSE]
    assert proofs == ref["by_division"]
    assert proofs == ref["direct"]
    assert len(set(proofs)) == 128


SHAPES = {
    "X^4095": [0] * 4095 + [1],                                     # c_i[0]: the top of the gather's range
    "X^64": [0] * 64 + [1],                                         # the lowest coefficient that matters
    "degree 200": [_rnd.randrange(1, R) for _ in range(201)],       # H_0 .. H_2
    "degree 63": [_rnd.randrange(1, R) for _ in range(64)],         # below X^64: every quotient is zero
    "constant": [9],
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_where_the_indexing_can_go_wrong(host, name):
    coeffs = SHAPES[name]
    rc, cells, proofs, st = c_call(host.engine.h, [S.coefficients_to_blob(coeffs)])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    want_cells = S.compute_cells(coeffs)
    assert cells[0] == want_cells and all(any(c) for c in want_cells)      # the cells are not trivial even where the proofs are
    want = [commit(host, S.cell_quotient(coeffs, i)[0]) for i in ALL]
    assert proofs[0] == want
    if name == "X^64":
        assert proofs[0] == [SETUP_G1[0]] * 128
    if name in ("degree 63", "constant"):
        assert proofs[0] == [INF] * 128
    if name in ("X^4095", "degree 200"):
        assert len(set(proofs[0])) == 128


def test_degree_70_has_only_h0_so_all_proofs_are_equal(ref):
    cells, proofs = ref["single"][LOW]
    assert cells == CELLS[LOW]
    assert proofs == [ref["low"]] * 128 and ref["low"] != INF


def test_accepted_by_the_cell_verifier_and_rejected_when_rotated(host, ref):
    cells, proofs = ref["single"][DENSE]
    comm = host.g1_lincomb(COEFFS[DENSE])
    assert host.verify_cell_kzg_proof_batch([comm] * 128, ALL, cells, proofs) is True
    assert host.verify_cell_kzg_proof_batch([comm] * 128, ALL, cells, proofs[1:] + proofs[:1]) is False


def test_three_blobs_in_one_call_with_a_rejected_one_in_the_middle(host, ref):
    elem_r = BLOBS[LOW][:32 * 70] + R.to_bytes(32, "big") + BLOBS[LOW][32 * 71:]
    rc, cells, proofs, st = c_call(host.engine.h, [BLOBS[LOW], elem_r, BLOBS[DENSE]])
    assert (rc, st) == (N.LB_OK, [N.LB_OK, N.LB_BAD_SCALAR, N.LB_OK])
    assert cells[1] == [bytes(2048)] * 128 and proofs[1] == [bytes(48)] * 128
    assert (cells[0], proofs[0]) == ref["single"][LOW]
    assert (cells[2], proofs[2]) == ref["single"][DENSE]


def _load(lib, h, n_g2, g1=SETUP_G1):
    g1b, g2b = np.frombuffer(b"".join(g1), np.uint8), np.frombuffer(b"".join(SETUP_G2[:n_g2]), np.uint8)
    st = np.zeros(len(g1), np.int32)
    return lib.lb_kzg_load_setup(h, g1b.ctypes.data_as(U8), len(g1), g2b.ctypes.data_as(U8), n_g2, st.ctypes.data_as(I32))


def test_table_lifecycle_and_argument_errors(host, ref):
    from lodestar_amd.engine import Engine
    lib = N.load()
    h = host.engine.h
    assert lib.lb_kzg_compute_cells_and_proofs(h, 0, None, None, None, None) == N.LB_OK
    assert lib.lb_kzg_compute_cells_and_proofs(h, 129, None, None, None, None) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_compute_cells_and_proofs(h, 1, None, None, None, None) == N.LB_ERR_ARGUMENT
    want = ([ref["single"][LOW][0]], [ref["single"][LOW][1]], [N.LB_OK])
    with Engine(0) as fresh:
        assert c_call(fresh.h, [BLOBS[LOW]])[0] == N.LB_ERR_ARGUMENT            # no setup at all
        assert _load(lib, fresh.h, 2) == N.LB_OK                               # two G2 points: nothing here pairs
        assert c_call(fresh.h, [BLOBS[LOW]]) == (N.LB_OK,) + want              # the first call builds the table
        assert c_call(fresh.h, [BLOBS[LOW]]) == (N.LB_OK,) + want              # the second reuses it
        # another setup (the same points in reverse order: any G1 points load) drops the table: the proofs are
        # now commitments over THAT setup, by its own host-mode lb_g1_lincomb; a stale table would give the old ones
        assert _load(lib, fresh.h, 2, SETUP_G1[::-1]) == N.LB_OK
        q = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in S.cell_quotient(COEFFS[LOW], 0)[0]), np.uint8)
        out48 = np.zeros(48, np.uint8)
        assert lib.lb_g1_lincomb(fresh.h, len(q) // 32, None, q.ctypes.data_as(U8), out48.ctypes.data_as(U8)) == N.LB_OK
        rc, cells, proofs, st = c_call(fresh.h, [BLOBS[LOW]])
        assert (rc, st, cells) == (N.LB_OK, [N.LB_OK], want[0])
        assert proofs[0] == [out48.tobytes()] * 128 and out48.tobytes() != ref["low"]
        assert _load(lib, fresh.h, len(SETUP_G2)) == N.LB_OK                   # and back
        assert c_call(fresh.h, [BLOBS[LOW]]) == (N.LB_OK,) + want
        rc, cells, proofs, st = c_call(fresh.h, [BLOBS[DENSE]])
        assert (rc, st) == (N.LB_OK, [N.LB_OK]) and (cells[0], proofs[0]) == ref["single"][DENSE]


def test_python_surface(engine, host, ref):
    elem_r = R.to_bytes(32, "big") + BLOBS[LOW][32:]
    for kz in (host, K.Kzg(engine, field="device")):       # always the device call, whatever `field` is
        cells, proofs = kz.compute_cells_and_kzg_proofs(BLOBS[LOW])
        assert (cells, proofs) == ref["single"][LOW]
        got = kz.compute_cells_and_kzg_proofs_many([BLOBS[LOW], elem_r, BLOBS[DENSE]])
        assert got[0] == ref["single"][LOW] and got[2] == ref["single"][DENSE]
        assert isinstance(got[1], K.KzgError) and "BLST_BAD_SCALAR" in str(got[1])
        assert kz.computeCellsAndKzgProofs(BLOBS[LOW]) == ref["single"][LOW]
        assert kz.computeCellsAndKzgProofsMany([BLOBS[LOW]]) == [ref["single"][LOW]]
        with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
            kz.compute_cells_and_kzg_proofs(elem_r)
    assert host.compute_cells_and_kzg_proofs_many([]) == []
    with pytest.raises(ValueError):                        # a wrong blob length raises before anything is sent
        host.compute_cells_and_kzg_proofs(BLOBS[LOW][:-1])
    with pytest.raises(ValueError):
        host.compute_cells_and_kzg_proofs_many([BLOBS[LOW], b""])


def write_js_fixture(path, host):
    """the bytes tests/js/test_kzg_fk20.js checks the JS surface against (tests/test_js_kzg_fk20.py)"""
    cells, proofs = host.compute_cells_and_kzg_proofs(BLOBS[LOW])
    with open(path, "w") as f:
        json.dump({"blob": BLOBS[LOW].hex(), "cells": [c.hex() for c in cells], "proofs": [p.hex() for p in proofs]}, f)
