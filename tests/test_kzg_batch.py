"""lb_kzg_verify_aggregate_proof_batch: many blob sidecars verified in one pass (C ABI, Python
Kzg.verify_aggregate_kzg_proof_batch, the JS ckzg module's verifyAggregateKzgProofBatch).

Every expected verdict comes from the single call for that sidecar alone
(lb_kzg_verify_aggregate_proof / Kzg(engine, field="device").verifyAggregateKzgProof), from the host
path (Kzg(engine)), from oracle/kzg.py or from Python integers -- never from the batch call.  The
polynomial size is fixed at 4096 by the setup, so the shapes are sidecar counts, blob counts per
sidecar and positions.  The sidecars are built once per module from three base blobs: eight types
over different blob lists, so a sidecar checked against another's blobs, commitments or proof fails."""
import ctypes
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from lodestar_amd import _native as N
from lodestar_amd import kzg as K
from oracle import bls_oracle as o
from oracle import kzg as OK

pytestmark = pytest.mark.gpu

R = o.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = bytes([0xC0]) + bytes(47)
U8, U32, I32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)


def _blob_of(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def _sequential_blob(off=0):
    b = bytearray(K.BYTES_PER_BLOB)
    for i in range(K.FIELD_ELEMENTS_PER_BLOB):
        b[32 * i: 32 * i + 4] = ((i + off) & 0xFFFFFFFF).to_bytes(4, "big")
    return bytes(b)


def _dense_vals(seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(K.FIELD_ELEMENTS_PER_BLOB)]


def _off_subgroup_g1():
    """an on-curve G1 point outside the order-r subgroup (cofactor component), as in test_kzg_device.py"""
    x = 5
    while True:
        y = o.fp_sqrt((x * x * x + o.B1) % o.P)
        if y is not None and o.g1_mul((x, y), R) is not None:
            return (x, y)
        x += 1


BLOBS = [_sequential_blob(0), _sequential_blob(7), _blob_of(_dense_vals(41))]
TYPES = [(), (0,), (1,), (2,), (0, 1), (1, 0), (0, 2), (0, 1, 2)]


@pytest.fixture(scope="module")
def host(engine):
    return K.Kzg(engine)


@pytest.fixture(scope="module")
def dev(engine):
    return K.Kzg(engine, field="device")


@pytest.fixture(scope="module")
def cars(host, dev):
    """the eight sidecar types as (blobs, commitments, proof): commitments from the host path, proofs
    from computeAggregateKzgProof"""
    comms = [host.blob_to_kzg_commitment(b) for b in BLOBS]
    out = {}
    for t in TYPES:
        blobs = [BLOBS[i] for i in t]
        out[t] = (blobs, [comms[i] for i in t], dev.computeAggregateKzgProof(blobs))
    assert out[()][2] == INF
    return out


def c_batch(engine_h, sidecars, out=None):
    """the C call on a list of (blobs, commitments, proof); returns (rc, out_ok as a list)"""
    lib = N.load()
    offs, blobs, comms, proofs = [0], [], [], []
    for b, c, p in sidecars:
        blobs += list(b)
        comms += list(c)
        proofs.append(p)
        offs.append(len(blobs))
    n = len(sidecars)
    bl = np.frombuffer(b"".join(blobs) or b"\x00", np.uint8)
    cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
    pf = np.frombuffer(b"".join(proofs) or b"\x00", np.uint8)
    off = np.asarray(offs, np.uint32)
    if out is None:
        out = np.full(max(n, 1), -99, np.int32)
    rc = lib.lb_kzg_verify_aggregate_proof_batch(engine_h, n, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                 cm.ctypes.data_as(U8), pf.ctypes.data_as(U8), out.ctypes.data_as(I32))
    return rc, out.tolist()[:n]


def c_single(engine_h, sidecar):
    """what lb_kzg_verify_aggregate_proof reports for one sidecar: *ok, or -code where it returns a code"""
    lib = N.load()
    b, c, p = sidecar
    bl = np.frombuffer(b"".join(b) or b"\x00", np.uint8)
    cm = np.frombuffer(b"".join(c) or b"\x00", np.uint8)
    pb = (ctypes.c_uint8 * 48).from_buffer_copy(p)
    ok = ctypes.c_int32(-99)
    rc = lib.lb_kzg_verify_aggregate_proof(engine_h, len(b), bl.ctypes.data_as(U8), cm.ctypes.data_as(U8),
                                           ctypes.cast(pb, U8), ctypes.byref(ok))
    return ok.value if rc == N.LB_OK else -rc


def test_mixed_shapes(dev, cars):
    """offsets [0,0,1,3,3,4]: sidecars of 0, 1, 2, 0 and 1 blobs, all valid"""
    batch = [cars[()], cars[(2,)], cars[(1, 0)], cars[()], cars[(0,)]]
    rc, got = c_batch(dev.engine.h, batch)
    assert rc == N.LB_OK
    assert got == [1] * 5
    assert got == [c_single(dev.engine.h, s) for s in batch]


def test_no_sidecars_writes_nothing(dev):
    out = np.full(4, -77, np.int32)
    rc, _ = c_batch(dev.engine.h, [], out=out)
    assert rc == N.LB_OK
    assert out.tolist() == [-77] * 4
    lib = N.load()
    assert lib.lb_kzg_verify_aggregate_proof_batch(dev.engine.h, 0, None, None, None, None, None) == N.LB_OK


def test_position_specific_verdicts_across_a_block_boundary(dev, cars):
    """33 sidecars cycling through the eight types (48 blobs + 66 more points: more than one
    block of the one k_g1_terms launch), with defects at positions 0, 17, 31 and 32"""
    batch = [cars[TYPES[k % 8]] for k in range(33)]
    # positions 0 and 32 are the empty type: another sidecar's proof
    batch[0] = ([], [], cars[(0,)][2])
    batch[32] = ([], [], cars[(0, 1)][2])
    b, c, p = batch[17]                       # type (0,): a blob byte flipped
    bad = bytearray(b[0])
    bad[32 * 100 + 31] ^= 1
    batch[17] = ([bytes(bad)], c, p)
    b, c, p = batch[31]                       # type (0, 1, 2): commitments swapped
    batch[31] = (b, [c[1], c[0], c[2]], p)
    rc, got = c_batch(dev.engine.h, batch)
    assert rc == N.LB_OK
    assert got == [c_single(dev.engine.h, s) for s in batch]
    assert got == [0 if k in (0, 17, 31, 32) else 1 for k in range(33)]


def test_rejections_stay_local(dev, cars):
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r = bytearray(BLOBS[1])
    elem_r[32 * 4095: 32 * 4096] = R.to_bytes(32, "big")     # the last element equal to r
    elem_r = bytes(elem_r)
    flagless = bytearray(cars[(0, 2)][2])
    flagless[0] &= 0x7F                                       # compression flag cleared
    good = [cars[(0, 1)], cars[(2,)], cars[(0, 1, 2)], cars[(1, 0)]]
    defects = [
        (([BLOBS[0], elem_r], cars[(0, 1)][1], cars[(0, 1)][2]), -N.LB_BAD_SCALAR),
        ((cars[(1, 0)][0], [cars[(1, 0)][1][0], off_g1], cars[(1, 0)][2]), -N.LB_POINT_NOT_IN_GROUP),
        ((cars[(0, 1)][0], cars[(0, 1)][1], off_g1), -N.LB_POINT_NOT_IN_GROUP),
        ((cars[(0, 2)][0], cars[(0, 2)][1], bytes(flagless)), None),   # the decode code the single call gives
        (([], [], cars[(1,)][2]), 0),
        (([], [], INF), 1),
        (([elem_r, BLOBS[0]], [off_g1, cars[(0,)][1][0]], cars[(0, 1)][2]), -N.LB_BAD_SCALAR),
    ]
    batch, expect = [], []
    for i, (s, exp) in enumerate(defects):
        batch += [good[i % len(good)], s]
        expect += [1, exp]
    batch.append(good[0])
    expect.append(1)
    singles = [c_single(dev.engine.h, s) for s in batch]
    k_flag = 2 * 3 + 1
    assert singles[k_flag] < 0 and singles[k_flag] not in (-N.LB_POINT_NOT_IN_GROUP, -N.LB_BAD_SCALAR)
    expect[k_flag] = singles[k_flag]
    assert singles == expect
    rc, got = c_batch(dev.engine.h, batch)
    assert rc == N.LB_OK
    assert got == expect


def test_exactly_one_point_at_infinity_rejects(dev, cars):
    """a one-blob sidecar whose proof is the point at infinity although its polynomial is not constant:
    P is infinity, T = C - [y] G1 is not, and e(T, -G2) alone is not 1.  (The other way round, T at
    infinity under a finite proof, would need C = [y] G1 - [x] pi with x hashed from C; both at
    infinity is the empty sidecar of test_rejections_stay_local.)"""
    blobs, comms, proof = cars[(0,)]
    assert proof != INF
    rc, got = c_batch(dev.engine.h, [(blobs, comms, INF)])
    assert (rc, got) == (N.LB_OK, [0])
    assert c_single(dev.engine.h, (blobs, comms, INF)) == 0


def test_argument_errors(dev, cars):
    from lodestar_amd.engine import Engine
    lib = N.load()
    h = dev.engine.h
    b, c, p = cars[(0,)]
    bl, cm, pf = (np.frombuffer(x, np.uint8) for x in (b[0], c[0], p))
    out = np.full(2, -99, np.int32)

    def call(eh, n, offs, out_ptr=out.ctypes.data_as(I32), proofs=pf):
        off = np.asarray(offs, np.uint32)
        return lib.lb_kzg_verify_aggregate_proof_batch(eh, n, off.ctypes.data_as(U32), bl.ctypes.data_as(U8),
                                                       cm.ctypes.data_as(U8), proofs.ctypes.data_as(U8), out_ptr)

    assert call(h, 1, [0, 1]) == N.LB_OK and out[0] == 1
    with Engine(0) as fresh:   # no setup loaded on this engine
        assert call(fresh.h, 1, [0, 1]) == N.LB_ERR_ARGUMENT
    assert call(h, 1, [1, 1]) == N.LB_ERR_ARGUMENT
    two = np.frombuffer(p + p, np.uint8)
    assert call(h, 2, [0, 1, 0], proofs=two) == N.LB_ERR_ARGUMENT
    many = np.frombuffer(INF * 1025, np.uint8)
    big_out = np.full(1025, -99, np.int32)
    assert call(h, 1025, [0] * 1026, out_ptr=big_out.ctypes.data_as(I32), proofs=many) == N.LB_ERR_ARGUMENT
    assert big_out.tolist() == [-99] * 1025
    assert call(h, 1, [0, 1], out_ptr=None) == N.LB_ERR_ARGUMENT


def test_python_surface(dev, host, cars):
    off_g1 = o.g1_compress(_off_subgroup_g1())
    elem_r = _blob_of([R] + [0] * 4095)
    b01, c01, p01 = cars[(0, 1)]
    batch = [
        cars[(0, 1, 2)],
        (b01, c01, cars[(0,)][2]),                    # another sidecar's proof
        ([elem_r], cars[(0,)][1], cars[(0,)][2]),
        (b01, [c01[0], off_g1], p01),
        cars[()],
    ]
    for kz in (dev, host):    # available whatever `field` is
        got = kz.verify_aggregate_kzg_proof_batch(batch)
        assert got[0] is True and got[1] is False and got[4] is True
        for k in (2, 3):
            assert isinstance(got[k], K.KzgError)
            with pytest.raises(K.KzgError) as single:
                dev.verifyAggregateKzgProof(*batch[k])
            assert str(got[k]) == str(single.value)
        assert "BLST_BAD_SCALAR" in str(got[2]) and "BLST_POINT_NOT_IN_GROUP" in str(got[3])
    assert dev.verifyAggregateKzgProofBatch([]) == []
    # one valid sidecar against the host path
    assert host.verifyAggregateKzgProof(*cars[(0, 1, 2)]) is True
    assert host.verifyAggregateKzgProof(*batch[1]) is False
    # malformed input raises before anything is sent
    with pytest.raises(K.KzgError):
        dev.verifyAggregateKzgProofBatch([cars[(0,)], (b01, c01[:1], p01)])
    with pytest.raises(ValueError):
        dev.verifyAggregateKzgProofBatch([([b01[0][:-1]], c01[:1], p01)])
    with pytest.raises(K.KzgError):
        dev.verifyAggregateKzgProofBatch([(b01, [c01[0], c01[1][:47]], p01)])
    with pytest.raises(K.KzgError):
        dev.verifyAggregateKzgProofBatch([(b01, c01, p01 + b"\x00")])


def test_one_blob_sidecar_against_the_oracle_pairing(dev, cars):
    """one sidecar of one blob: with one blob the aggregate is the blob (r^0 = 1), so the check is
    verify_kzg_proof_impl(C, x, y, proof) with x from the oracle's transcript and y the oracle's
    evaluation -- this file's one pure-Python pairing"""
    _, g2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
    blobs, comms, proof = cars[(2,)]
    vals = K.blob_to_polynomial(blobs[0])
    _, x = OK.compute_challenges([vals], comms)
    y = OK.evaluate_polynomial_in_evaluation_form(vals, x, K.ROOTS_BRP)
    expected = bool(OK.verify_kzg_proof_impl(comms[0], x, y, proof, g2))
    assert expected is True
    assert dev.verifyAggregateKzgProofBatch([cars[(2,)]]) == [expected]


def test_js_batch_matches_js_single_calls():
    """tests/js/test_kzg_batch.js: verifyAggregateKzgProofBatch of the JS ckzg surface in both field
    modes, each verdict equal to the JS single call's"""
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "test_kzg_batch.js")], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "js kzg batch ok", r.stdout
    assert json.loads(lines[-2])[:3] == [False, True, False]
