"""The per-blob (Deneb) KZG calls on the GPU: lb_kzg_compute_blob_proofs and
lb_kzg_verify_blob_proof_batch (C ABI), and the Python surface over them (Kzg.compute_blob_kzg_proof,
verify_blob_kzg_proof, verify_blob_kzg_proof_batch(_many), compute_kzg_proof_bytes,
verify_kzg_proof_bytes).

Expected values never come from the calls under test: proofs from host-mode Python (Python field
work over lb_g1_lincomb), verdicts from tests/kzg_deneb_spec.py's batch equation evaluated through
the host-mode group calls (lb_g1_lincomb, lb_kzg_verify_proof) or, once, the pure-Python pairing.
The polynomial size is fixed at 4096 by the setup, so the shapes are group counts and blobs per
group: groups of 0, 1, 2, 0 and 3 blobs, six blobs in all, built once per module."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_deneb_spec as S  # noqa: E402
from test_kzg_batch import _off_subgroup_g1  # noqa: E402

from lodestar_amd import _native as N  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402
from oracle import bls_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

R = o.R
INF = bytes([0xC0]) + bytes(47)
U8, U32, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
SIZES = [0, 1, 2, 0, 3]
OFFSETS = [0, 0, 1, 3, 3, 6]
LOW_DEGREE = [5, 3, 0, 2]


def _blob_of(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def _sequential_blob(off=0):
    return _blob_of([(i + off) & 0xFFFFFFFF for i in range(K.FIELD_ELEMENTS_PER_BLOB)])


def _dense_blob(seed):
    rnd = random.Random(seed)
    return _blob_of([rnd.randrange(R) for _ in range(K.FIELD_ELEMENTS_PER_BLOB)])


# blob 0: the one-blob group (low degree, for the Python pairing); 1, 2: the two-blob group;
# 3, 4, 5: the three-blob group, 4 a constant polynomial (its proof is the point at infinity)
BLOBS = [S.low_degree_blob(LOW_DEGREE), _dense_blob(77), _sequential_blob(0),
         _sequential_blob(7), _blob_of([9] * K.FIELD_ELEMENTS_PER_BLOB), _dense_blob(78)]
CONSTANT = 4


@pytest.fixture(scope="module")
def host(engine):
    return K.Kzg(engine)


@pytest.fixture(scope="module")
def dev(engine):
    return K.Kzg(engine, field="device")


def c_compute(engine_h, blobs, comms):
    lib = N.load()
    n = len(blobs)
    bl = np.frombuffer(b"".join(blobs), np.uint8)
    cm = np.frombuffer(b"".join(comms), np.uint8)
    out = np.full(48 * n, 0xEE, np.uint8)
    st = np.full(n, -99, np.int32)
    rc = lib.lb_kzg_compute_blob_proofs(engine_h, n, bl.ctypes.data_as(U8), cm.ctypes.data_as(U8), out.ctypes.data_as(U8),
                                        st.ctypes.data_as(I32))
    return rc, [out[48 * b: 48 * b + 48].tobytes() for b in range(n)], st.tolist()


def c_verify(engine_h, blobs, comms, proofs, offsets=OFFSETS):
    """the C call over flat lists; returns (rc, out_ok as a list)"""
    lib = N.load()
    n = len(offsets) - 1
    bl = np.frombuffer(b"".join(blobs) or b"\x00", np.uint8)
    cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
    pf = np.frombuffer(b"".join(proofs) or b"\x00", np.uint8)
    off = np.asarray(offsets, np.uint32)
    out = np.full(max(n, 1), -99, np.int32)
    rc = lib.lb_kzg_verify_blob_proof_batch(engine_h, n, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                            cm.ctypes.data_as(U8), pf.ctypes.data_as(U8), out.ctypes.data_as(I32))
    return rc, out.tolist()[:n]


@pytest.fixture(scope="module")
def ref(host, dev):
    """commitments (the existing device call), proofs (the C call under test, checked against host
    mode below), and z_i, y_i from the helper's transcript and host-mode Python integers"""
    comms = dev._device_commitments(BLOBS)
    rc, proofs, st = c_compute(dev.engine.h, BLOBS, comms)
    assert rc == N.LB_OK and st == [N.LB_OK] * 6
    zs = [S.compute_challenge(b, c) for b, c in zip(BLOBS, comms)]
    ys = [K.evaluate_coefficients(K.evaluations_to_coefficients(K.blob_to_polynomial(b)), z) for b, z in zip(BLOBS, zs)]
    return {"comms": comms, "proofs": proofs, "zs": zs, "ys": ys}


def _expected(host, ref, blobs, comms, proofs, offsets=OFFSETS):
    """the helper's batch equation per group, its two linear combinations and its pairing product
    through the host-mode group calls; z and y recomputed where a blob or commitment differs"""
    out = []
    for k in range(len(offsets) - 1):
        idx = range(offsets[k], offsets[k + 1])
        zs, ys = [], []
        for j in idx:
            if blobs[j] is BLOBS[j] and comms[j] is ref["comms"][j]:
                zs.append(ref["zs"][j])
                ys.append(ref["ys"][j])
            else:
                zs.append(S.compute_challenge(blobs[j], comms[j]))
                ys.append(K.evaluate_coefficients(K.evaluations_to_coefficients(K.blob_to_polynomial(blobs[j])), zs[-1]))
        out.append(1 if S.batch_equation([comms[j] for j in idx], zs, ys, [proofs[j] for j in idx], None,
                                         lincomb=lambda pts, sc: host.g1_lincomb(sc, pts),
                                         pairing_check=lambda t, p: host.verify_kzg_proof(t, 0, 0, p)) else 0)
    return out


def test_proofs_equal_host_mode(host, dev, ref):
    """dense, sequential and constant blobs: the C call's proofs are host-mode Python's bytes"""
    for j in (1, 2, CONSTANT):
        assert ref["proofs"][j] == host.compute_blob_kzg_proof(BLOBS[j], ref["comms"][j]), j
    assert ref["proofs"][CONSTANT] == INF
    assert dev.compute_blob_kzg_proof(BLOBS[1], ref["comms"][1]) == ref["proofs"][1]
    assert S.evaluate_blob(BLOBS[1], ref["zs"][1]) == ref["ys"][1]      # the helper's own evaluation agrees
    # an infinity commitment is allowed (a wrong one: the proof is still that of p at its z)
    rc, proofs, st = c_compute(dev.engine.h, [BLOBS[2]], [INF])
    assert rc == N.LB_OK and st == [N.LB_OK]
    assert proofs[0] == host.compute_blob_kzg_proof(BLOBS[2], INF)


def test_compute_rejections(dev, ref):
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r = BLOBS[2][:-32] + R.to_bytes(32, "big")
    comms = ref["comms"]
    rc, proofs, st = c_compute(dev.engine.h, [BLOBS[1], elem_r, BLOBS[3], elem_r], [comms[1], comms[2], off_g1, off_g1])
    assert rc == N.LB_OK
    assert st == [N.LB_OK, N.LB_BAD_SCALAR, N.LB_POINT_NOT_IN_GROUP, N.LB_POINT_NOT_IN_GROUP]
    assert proofs[0] == ref["proofs"][1]
    assert proofs[1] == proofs[2] == proofs[3] == bytes(48)
    with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
        dev.compute_blob_kzg_proof(elem_r, comms[2])
    with pytest.raises(K.KzgError, match="BLST_POINT_NOT_IN_GROUP"):
        dev.compute_blob_kzg_proof(BLOBS[3], off_g1)
    lib = N.load()
    assert lib.lb_kzg_compute_blob_proofs(dev.engine.h, 0, None, None, None, None) == N.LB_OK


def test_all_groups_accepted(host, dev, ref, monkeypatch):
    rc, got = c_verify(dev.engine.h, BLOBS, ref["comms"], ref["proofs"])
    assert rc == N.LB_OK
    assert got == [1] * 5
    assert got == _expected(host, ref, BLOBS, ref["comms"], ref["proofs"])
    lib = N.load()
    assert lib.lb_kzg_batch_hash_ns(dev.engine.h) > 0
    monkeypatch.setenv("LB_KZG_HASH_THREADS", "1")      # one hashing thread: the same verdicts
    assert c_verify(dev.engine.h, BLOBS, ref["comms"], ref["proofs"]) == (N.LB_OK, [1] * 5)
    # constant blobs with infinity proofs alone: T and P both at infinity
    const = BLOBS[CONSTANT]
    assert c_verify(dev.engine.h, [const, const], [ref["comms"][CONSTANT]] * 2, [INF, INF], [0, 2]) == (N.LB_OK, [1])


def test_exactly_one_point_at_infinity_rejects(dev, ref):
    """a one-blob group whose proof is the point at infinity although its polynomial is not constant:
    P is infinity, T = C - [y] G1 is not, and e(T, -G2) alone is not 1.  (The other way round, T at
    infinity under a finite P, would need C = [y] G1 - [z] pi with z hashed from C.)"""
    assert ref["proofs"][1] != INF
    assert c_verify(dev.engine.h, [BLOBS[1]], [ref["comms"][1]], [INF], [0, 1]) == (N.LB_OK, [0])


def test_rejections_stay_local(host, dev, ref):
    comms, proofs = ref["comms"], ref["proofs"]
    h = dev.engine.h
    off_g1 = o.g1_compress(_off_subgroup_g1())
    flagless = bytearray(comms[4])
    flagless[0] &= 0x7F                                   # compression flag cleared
    flagless = bytes(flagless)
    lib = N.load()
    one = (ctypes.c_uint8 * 32)(1)
    out48 = (ctypes.c_uint8 * 48)()
    bad_code = lib.lb_g1_lincomb(h, 1, ctypes.cast((ctypes.c_uint8 * 48).from_buffer_copy(flagless), U8),
                                 ctypes.cast(one, U8), ctypes.cast(out48, U8))   # the decode code of the existing call
    assert bad_code not in (N.LB_OK, N.LB_POINT_NOT_IN_GROUP, N.LB_BAD_SCALAR)

    def sub(lst, j, v):
        return lst[:j] + [v] + lst[j + 1:]

    # a tampered proof in the three-blob group (a valid G1 point: another blob's proof)
    p = sub(proofs, 5, proofs[1])
    assert c_verify(h, BLOBS, comms, p) == (N.LB_OK, [1, 1, 1, 1, 0])
    assert _expected(host, ref, BLOBS, comms, p) == [1, 1, 1, 1, 0]
    # two proofs swapped inside the two-blob group
    p = sub(sub(proofs, 1, proofs[2]), 2, proofs[1])
    assert c_verify(h, BLOBS, comms, p) == (N.LB_OK, [1, 1, 0, 1, 1])
    assert _expected(host, ref, BLOBS, comms, p) == [1, 1, 0, 1, 1]
    # a blob element equal to r
    elem_r = BLOBS[2][:-32] + R.to_bytes(32, "big")
    assert c_verify(h, sub(BLOBS, 2, elem_r), comms, proofs) == (N.LB_OK, [1, 1, -N.LB_BAD_SCALAR, 1, 1])
    # points outside the subgroup, a bad encoding: commitments and proofs
    assert c_verify(h, BLOBS, sub(comms, 0, off_g1), proofs) == (N.LB_OK, [1, -N.LB_POINT_NOT_IN_GROUP, 1, 1, 1])
    assert c_verify(h, BLOBS, comms, sub(proofs, 4, off_g1)) == (N.LB_OK, [1, 1, 1, 1, -N.LB_POINT_NOT_IN_GROUP])
    assert c_verify(h, BLOBS, sub(comms, 4, flagless), proofs) == (N.LB_OK, [1, 1, 1, 1, -bad_code])
    assert c_verify(h, BLOBS, comms, sub(proofs, 1, flagless)) == (N.LB_OK, [1, 1, -bad_code, 1, 1])


def test_precedence_across_two_errors(dev, ref):
    comms, proofs = ref["comms"], ref["proofs"]
    h = dev.engine.h
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r4 = R.to_bytes(32, "big") + BLOBS[4][32:]
    blobs4 = BLOBS[:4] + [elem_r4] + BLOBS[5:]

    def group3(c, p, blobs=blobs4):
        rc, got = c_verify(h, blobs, c, p)
        assert rc == N.LB_OK and got[:4] == [1] * 4
        return got[4]

    # the lower blob wins: blob 4's element before blob 5's commitment
    assert group3(comms[:5] + [off_g1], proofs) == -N.LB_BAD_SCALAR
    # ... and blob 3's proof before blob 4's element
    assert group3(comms, proofs[:3] + [off_g1] + proofs[4:]) == -N.LB_POINT_NOT_IN_GROUP
    # within blob 4: commitment, then element, then proof
    assert group3(comms[:4] + [off_g1] + comms[5:], proofs) == -N.LB_POINT_NOT_IN_GROUP
    assert group3(comms, proofs[:4] + [off_g1] + proofs[5:]) == -N.LB_BAD_SCALAR
    assert group3(comms, proofs[:4] + [off_g1] + proofs[5:], blobs=BLOBS) == -N.LB_POINT_NOT_IN_GROUP


def test_low_degree_group_against_the_python_pairing(dev, ref):
    """the one-blob group: proof and verdict against the oracle alone -- this file's one pure-Python
    pairing"""
    g1, g2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
    blob, c, z, y, proof = S.low_degree_proof(g1, LOW_DEGREE)
    assert (blob, c, proof) == (BLOBS[0], ref["comms"][0], ref["proofs"][0])
    assert (z, y) == (ref["zs"][0], ref["ys"][0])
    expected = S.batch_equation([c], [z], [y], [proof], g2)
    assert expected is True
    assert c_verify(dev.engine.h, [blob], [c], [proof], [0, 1]) == (N.LB_OK, [1])
    assert dev.verify_blob_kzg_proof(blob, c, proof) is expected


def test_argument_errors(dev, ref):
    from lodestar_amd.engine import Engine
    h = dev.engine.h
    one = ([BLOBS[0]], [ref["comms"][0]], [ref["proofs"][0]])
    assert c_verify(h, *one, [0, 1]) == (N.LB_OK, [1])
    with Engine(0) as fresh:   # no setup loaded on this engine
        assert c_verify(fresh.h, *one, [0, 1])[0] == N.LB_ERR_ARGUMENT
        assert c_compute(fresh.h, one[0], one[1])[0] == N.LB_ERR_ARGUMENT
    assert c_verify(h, *one, [1, 1])[0] == N.LB_ERR_ARGUMENT
    assert c_verify(h, *one, [0, 1, 0])[0] == N.LB_ERR_ARGUMENT
    assert c_verify(h, *one, [0] * 1026) == (N.LB_ERR_ARGUMENT, [-99] * 1025)
    assert c_verify(h, *one, [0, 1025])[0] == N.LB_ERR_ARGUMENT      # rejected before any blob is read
    lib = N.load()
    off = np.asarray([0, 1], np.uint32)
    bl, cm, pf = (np.frombuffer(x[0], np.uint8) for x in one)
    assert lib.lb_kzg_verify_blob_proof_batch(h, 1, off.ctypes.data_as(U32), bl.ctypes.data_as(U8), cm.ctypes.data_as(U8),
                                              pf.ctypes.data_as(U8), None) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_verify_blob_proof_batch(h, 1, off.ctypes.data_as(U32), bl.ctypes.data_as(U8), cm.ctypes.data_as(U8),
                                              None, np.zeros(1, np.int32).ctypes.data_as(I32)) == N.LB_ERR_ARGUMENT
    assert lib.lb_kzg_verify_blob_proof_batch(h, 0, None, None, None, None, None) == N.LB_OK
    assert lib.lb_kzg_compute_blob_proofs(h, 1025, bl.ctypes.data_as(U8), cm.ctypes.data_as(U8), None, None) == N.LB_ERR_ARGUMENT


def test_point_proofs_as_bytes(dev, host, ref):
    """computeKzgProof / verifyKzgProof: z and y as 32 big-endian bytes, each below r"""
    z = (0x1234 << 200) + 5
    zb = z.to_bytes(32, "big")
    proof, yb = dev.compute_kzg_proof_bytes(BLOBS[2], zb)
    assert (proof, yb) == host.compute_kzg_proof_bytes(BLOBS[2], zb)
    assert int.from_bytes(yb, "big") == S.evaluate_blob(BLOBS[2], z)
    assert dev.verify_kzg_proof_bytes(ref["comms"][2], zb, yb, proof) is True
    assert dev.verify_kzg_proof_bytes(ref["comms"][2], zb, (1).to_bytes(32, "big"), proof) is False
    rb = R.to_bytes(32, "big")
    with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
        dev.verify_kzg_proof_bytes(ref["comms"][2], rb, yb, proof)
    with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
        dev.verifyKzgProof(ref["comms"][2], zb, rb, proof)
    with pytest.raises(K.KzgError):
        dev.computeKzgProof(BLOBS[2], rb)
    with pytest.raises(K.KzgError):
        dev.verify_kzg_proof_bytes(ref["comms"][2], zb[1:], yb, proof)


def test_python_surface(dev, host, ref):
    comms, proofs = ref["comms"], ref["proofs"]
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r = R.to_bytes(32, "big") + BLOBS[1][32:]
    groups = [
        (BLOBS[3:6], comms[3:6], proofs[3:6]),
        (BLOBS[1:3], comms[1:3], [proofs[2], proofs[1]]),
        ([elem_r, BLOBS[2]], comms[1:3], proofs[1:3]),
        (BLOBS[1:3], [comms[1], off_g1], proofs[1:3]),
        ([], [], []),
    ]
    for kz in (dev, host):    # the batch calls use the device call whatever `field` is
        got = kz.verify_blob_kzg_proof_batch_many(groups)
        assert got[0] is True and got[1] is False and got[4] is True
        assert isinstance(got[2], K.KzgError) and "BLST_BAD_SCALAR" in str(got[2])
        assert isinstance(got[3], K.KzgError) and "BLST_POINT_NOT_IN_GROUP" in str(got[3])
        assert kz.verifyBlobKzgProofBatch(*groups[0]) is True
        assert kz.verifyBlobKzgProofBatch(*groups[1]) is False
        assert kz.verifyBlobKzgProofBatch([], [], []) is True
        with pytest.raises(K.KzgError, match="BLST_BAD_SCALAR"):
            kz.verifyBlobKzgProofBatch(*groups[2])
    assert dev.verifyBlobKzgProofBatchMany([]) == []
    # the single call in both field modes
    for kz in (dev, host):
        assert kz.verifyBlobKzgProof(BLOBS[2], comms[2], proofs[2]) is True
        assert kz.verifyBlobKzgProof(BLOBS[2], comms[2], proofs[1]) is False
        with pytest.raises(K.KzgError, match="BLST_POINT_NOT_IN_GROUP"):
            kz.verifyBlobKzgProof(BLOBS[2], off_g1, proofs[2])
    # malformed input raises before anything is sent
    with pytest.raises(K.KzgError):
        dev.verifyBlobKzgProofBatch(BLOBS[1:3], comms[1:3], proofs[1:2])
    with pytest.raises(ValueError):
        dev.verifyBlobKzgProofBatch([BLOBS[1][:-1]], comms[1:2], proofs[1:2])
    with pytest.raises(K.KzgError):
        dev.verifyBlobKzgProofBatch(BLOBS[1:2], [comms[1][:47]], proofs[1:2])
    with pytest.raises(K.KzgError):
        dev.computeBlobKzgProof(BLOBS[1], comms[1] + b"\x00")
