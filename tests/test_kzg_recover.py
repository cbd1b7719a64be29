"""lb_kzg_recover_cells_and_proofs (c-kzg recoverCellsAndKzgProofs) on the GPU, and the Python
surface over it (Kzg.recover_cells_and_kzg_proofs(_many) and the ckzg aliases).

Expected values never come from the call under test: cells from tests/kzg_cells_spec.py's Python
transform, proofs from lb_kzg_compute_cells_and_proofs on the original blob (FK20 from the blob's
bytes, pinned by tests/test_kzg_fk20.py); acceptance by the existing cell verifier.  The dense blob
and the degree-70 blob are those of tests/test_kzg_cells.py; the references are built once per module.
One blob is the smallest shape: each call is about one FK20 pass."""
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
U8, U32, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
ALL = list(range(128))
ZERO_OUT = ([bytes(2048)] * 128, [bytes(48)] * 128)
INDEX_SETS = {"0..63": list(range(64)), "64..127": list(range(64, 128)), "evens": list(range(0, 128, 2)),
              "odds": list(range(1, 128, 2)), "random 64": sorted(random.Random(64).sample(range(128), 64)),
              "random 65": sorted(random.Random(65).sample(range(128), 65)), "all but 0": list(range(1, 128)),
              "all but 127": list(range(127)), "all 128": list(range(128))}
SETUP_G1, SETUP_G2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
SHAPES = {"X^4095": [0] * 4095 + [1], "constant": [9]}
SHAPE_CELLS = {name: S.compute_cells(c) for name, c in SHAPES.items()}


def c_call(engine_h, groups, lib=None):
    """the C call over [(cell indices, cells)] per blob; returns (rc, per blob its 128 cells, per blob
    its 128 proofs, statuses)"""
    lib = lib or N.load()
    n = len(groups)
    off = np.cumsum([0] + [len(idx) for idx, _ in groups]).astype(np.uint32)
    ci = np.asarray([i for idx, _ in groups for i in idx] or [0], np.uint32)
    src = np.frombuffer(b"".join(c for _, cells in groups for c in cells) or b"\x00", np.uint8)
    cells = np.full(n * 128 * 2048, 0xEE, np.uint8)
    proofs = np.full(n * 128 * 48, 0xEE, np.uint8)
    st = np.full(n, -99, np.int32)
    rc = lib.lb_kzg_recover_cells_and_proofs(engine_h, n, off.ctypes.data_as(U32), ci.ctypes.data_as(U32), src.ctypes.data_as(U8),
                                             cells.ctypes.data_as(U8), proofs.ctypes.data_as(U8), st.ctypes.data_as(I32))
    craw, praw = cells.tobytes(), proofs.tobytes()
    return (rc, [[craw[(128 * b + i) * 2048: (128 * b + i + 1) * 2048] for i in ALL] for b in range(n)],
            [[praw[(128 * b + i) * 48: (128 * b + i + 1) * 48] for i in ALL] for b in range(n)], st.tolist())


def fk20(engine_h, blob):
    """the proofs of the original blob by lb_kzg_compute_cells_and_proofs"""
    from test_kzg_fk20 import c_call as fk_call
    rc, _, proofs, st = fk_call(engine_h, [blob])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    return proofs[0]


def given(cells, idx):
    return (list(idx), [cells[i] for i in idx])


def changed(cells, idx, which=3, elem=17):
    """the given cells with one element changed (still below r)"""
    idx, out = given(cells, idx)
    v = (int.from_bytes(out[which][32 * elem: 32 * elem + 32], "big") + 1) % R
    out[which] = out[which][:32 * elem] + v.to_bytes(32, "big") + out[which][32 * elem + 32:]
    return idx, out


@pytest.fixture(scope="module")
def host(engine):
    return K.Kzg(engine)


@pytest.fixture(scope="module")
def ref(host):
    """the reference proofs, computed once and never changed: FK20 on the original blobs"""
    h = host.engine.h
    out = {DENSE: fk20(h, BLOBS[DENSE]), LOW: fk20(h, BLOBS[LOW])}
    for name, coeffs in SHAPES.items():
        out[name] = fk20(h, S.coefficients_to_blob(coeffs))
    return out


@pytest.mark.parametrize("iset", list(INDEX_SETS))
def test_dense_blob_from_each_index_set(host, ref, iset):
    rc, cells, proofs, st = c_call(host.engine.h, [given(CELLS[DENSE], INDEX_SETS[iset])])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert cells[0] == CELLS[DENSE]
    assert proofs[0] == ref[DENSE] and len(set(proofs[0])) == 128


def test_degree_70_blob_from_the_first_half(host, ref):
    rc, cells, proofs, st = c_call(host.engine.h, [given(CELLS[LOW], INDEX_SETS["0..63"])])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert cells[0] == CELLS[LOW] and proofs[0] == ref[LOW]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_from_the_second_half(host, ref, name):
    rc, cells, proofs, st = c_call(host.engine.h, [given(SHAPE_CELLS[name], INDEX_SETS["64..127"])])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert cells[0] == SHAPE_CELLS[name] and proofs[0] == ref[name]
    if name == "constant":
        assert proofs[0] == [INF] * 128


def test_zero_blob(host):
    rc, cells, proofs, st = c_call(host.engine.h, [(INDEX_SETS["random 64"], [bytes(2048)] * 64)])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert cells[0] == [bytes(2048)] * 128 and proofs[0] == [INF] * 128


def test_accepted_by_the_cell_verifier(host):
    rc, cells, proofs, st = c_call(host.engine.h, [given(CELLS[DENSE], INDEX_SETS["odds"])])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    comm = host.g1_lincomb(COEFFS[DENSE])
    assert host.verify_cell_kzg_proof_batch([comm] * 128, ALL, cells[0], proofs[0]) is True


def test_three_blobs_in_one_call_with_a_rejected_one_in_the_middle(host, ref):
    h = host.engine.h
    hundred = sorted(random.Random(100).sample(range(128), 100))
    idx, bad = given(CELLS[LOW], hundred)
    bad[40] = bad[40][:32 * 5] + R.to_bytes(32, "big") + bad[40][32 * 6:]
    groups = [given(CELLS[DENSE], INDEX_SETS["random 64"]), (idx, bad), given(CELLS[LOW], ALL)]
    rc, cells, proofs, st = c_call(h, groups)
    assert (rc, st) == (N.LB_OK, [N.LB_OK, N.LB_BAD_SCALAR, N.LB_OK])
    assert (cells[1], proofs[1]) == ZERO_OUT
    for b in (0, 2):
        rc1, cells1, proofs1, st1 = c_call(h, [groups[b]])
        assert (rc1, st1) == (N.LB_OK, [N.LB_OK])
        assert (cells[b], proofs[b]) == (cells1[0], proofs1[0])
    assert (cells[0], proofs[0]) == (CELLS[DENSE], ref[DENSE])
    assert (cells[2], proofs[2]) == (CELLS[LOW], ref[LOW])


def test_a_changed_element_among_65_cells_is_rejected(host):
    rc, cells, proofs, st = c_call(host.engine.h, [changed(CELLS[DENSE], INDEX_SETS["random 65"])])
    assert (rc, st) == (N.LB_OK, [N.LB_VERIFY_FAIL])
    assert (cells[0], proofs[0]) == ZERO_OUT
    # an element >= r comes before the inconsistency
    idx, cs = changed(CELLS[DENSE], INDEX_SETS["random 65"])
    cs[64] = cs[64][:-32] + R.to_bytes(32, "big")
    rc, cells, proofs, st = c_call(host.engine.h, [(idx, cs)])
    assert (rc, st) == (N.LB_OK, [N.LB_BAD_SCALAR]) and (cells[0], proofs[0]) == ZERO_OUT


def test_a_changed_element_among_64_cells_is_another_blob(host):
    idx, cs = changed(CELLS[DENSE], INDEX_SETS["random 64"])
    rc, cells, proofs, st = c_call(host.engine.h, [(idx, cs)])
    assert (rc, st) == (N.LB_OK, [N.LB_OK])
    assert [cells[0][i] for i in idx] == cs
    assert cells[0] != CELLS[DENSE]


def _load(lib, h, n_g2):
    g1b, g2b = np.frombuffer(b"".join(SETUP_G1), np.uint8), np.frombuffer(b"".join(SETUP_G2[:n_g2]), np.uint8)
    st = np.zeros(len(SETUP_G1), np.int32)
    return lib.lb_kzg_load_setup(h, g1b.ctypes.data_as(U8), len(SETUP_G1), g2b.ctypes.data_as(U8), n_g2, st.ctypes.data_as(I32))


def test_argument_errors_and_a_setup_with_two_g2_points(host, ref):
    from lodestar_amd.engine import Engine
    lib = N.load()
    h = host.engine.h
    cells = CELLS[LOW]

    def rc_of(groups):
        rc, out_cells, _, st = c_call(h, groups)
        assert st == [-99] * len(groups) and out_cells[0][0] == b"\xEE" * 2048     # nothing written
        return rc

    assert rc_of([given(cells, range(63))]) == N.LB_ERR_ARGUMENT
    assert rc_of([(ALL + [128], cells + [cells[0]])]) == N.LB_ERR_ARGUMENT            # 129 cells
    assert rc_of([(list(range(63)) + [128], cells[:64])]) == N.LB_ERR_ARGUMENT        # index 128
    assert rc_of([(list(range(63)) + [62], cells[:63] + [cells[62]])]) == N.LB_ERR_ARGUMENT   # a duplicate
    assert rc_of([([1, 0] + list(range(2, 64)), [cells[1], cells[0]] + cells[2:64])]) == N.LB_ERR_ARGUMENT  # descending
    assert rc_of([given(cells, range(64)), given(cells, range(63))]) == N.LB_ERR_ARGUMENT
    off, ci = np.asarray([0, 64], np.uint32), np.arange(64, dtype=np.uint32)
    src = np.frombuffer(b"".join(cells[:64]), np.uint8)
    oc, op, st = np.zeros(128 * 2048, np.uint8), np.zeros(128 * 48, np.uint8), np.zeros(1, np.int32)
    args = [off.ctypes.data_as(U32), ci.ctypes.data_as(U32), src.ctypes.data_as(U8), oc.ctypes.data_as(U8), op.ctypes.data_as(U8),
            st.ctypes.data_as(I32)]
    assert lib.lb_kzg_recover_cells_and_proofs(h, 1, *args) == N.LB_OK
    for k in range(len(args)):                                                        # every pointer is needed
        assert lib.lb_kzg_recover_cells_and_proofs(h, 1, *(args[:k] + [None] + args[k + 1:])) == N.LB_ERR_ARGUMENT
    bad_off = np.asarray([1, 65], np.uint32)
    assert lib.lb_kzg_recover_cells_and_proofs(h, 1, bad_off.ctypes.data_as(U32), *args[1:]) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_recover_cells_and_proofs(h, 129, *args) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_recover_cells_and_proofs(h, 0, None, None, None, None, None, None) == N.LB_OK
    with Engine(0) as fresh:
        assert c_call(fresh.h, [given(cells, range(64))])[0] == N.LB_ERR_ARGUMENT     # no setup at all
        assert _load(lib, fresh.h, 2) == N.LB_OK                                      # two G2 points: nothing here pairs
        rc, out_cells, proofs, st = c_call(fresh.h, [given(cells, range(64))])        # this call builds the FK20 table
        assert (rc, st) == (N.LB_OK, [N.LB_OK])
        assert (out_cells[0], proofs[0]) == (CELLS[LOW], ref[LOW])


def test_python_surface(engine, host, ref):
    idx, cs = given(CELLS[LOW], INDEX_SETS["evens"])
    want = (CELLS[LOW], ref[LOW])
    bad = changed(CELLS[DENSE], INDEX_SETS["random 65"])
    elem_r = (idx, [R.to_bytes(32, "big") + cs[0][32:]] + cs[1:])
    for kz in (host, K.Kzg(engine, field="device")):       # always the device call, whatever `field` is
        assert kz.recover_cells_and_kzg_proofs(idx, cs) == want
        got = kz.recover_cells_and_kzg_proofs_many([(idx, cs), bad, elem_r, given(CELLS[DENSE], INDEX_SETS["0..63"])])
        assert got[0] == want and got[3] == (CELLS[DENSE], ref[DENSE])
        assert isinstance(got[1], K.KzgError) and "BLST_VERIFY_FAIL" in str(got[1])
        assert isinstance(got[2], K.KzgError) and "BLST_BAD_SCALAR" in str(got[2])
        assert kz.recoverCellsAndKzgProofs(idx, cs) == want
        assert kz.recoverCellsAndKzgProofsMany([(idx, cs)]) == [want]
        with pytest.raises(K.KzgError, match="BLST_VERIFY_FAIL"):
            kz.recover_cells_and_kzg_proofs(*bad)
    assert host.recover_cells_and_kzg_proofs_many([]) == []
    for bad_idx, bad_cells in [(idx, cs[:-1] + [cs[-1][:-1]]),                       # a wrong cell length
                               (idx[:-1], cs),                                       # lengths differ
                               (idx[:63], cs[:63]),                                  # too few
                               (ALL + [128], CELLS[LOW] + [cs[0]]),                  # too many
                               (idx[:63] + [128], cs), ([-1] + idx[1:], cs),         # a bad index
                               ([idx[1], idx[0]] + idx[2:], cs), (idx[:63] + [idx[62]], cs)]:   # unsorted, repeated
        with pytest.raises(ValueError):
            host.recover_cells_and_kzg_proofs(bad_idx, bad_cells)
        with pytest.raises(ValueError):
            host.recover_cells_and_kzg_proofs_many([(idx, cs), (bad_idx, bad_cells)])


def write_js_fixture(path, host):
    """the bytes tests/js/test_kzg_recover.js checks the JS surface against (tests/test_js_kzg_recover.py):
    the degree-70 blob's cells and its FK20 proofs"""
    with open(path, "w") as f:
        json.dump({"cells": [c.hex() for c in CELLS[LOW]], "proofs": [p.hex() for p in fk20(host.engine.h, BLOBS[LOW])]}, f)
