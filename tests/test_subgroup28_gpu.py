"""k_sig_subgroup on its limb-resident ladder (lb_curve.h g2_aff_in_subgroup28) against the 8-lane
form k_sig_subgroup_g8, whose arithmetic this change leaves alone, and against the oracle's
Signature.fromBytes(validate=true): one batch of 130 sets (two full waves and a 2-lane tail) holding
valid signatures, an infinity signature, a bad-size entry, a not-on-curve x, a bad encoding, curve
points outside G2, points of small order (orders 13 and 23: the ladder's acc == -P addition, its
run at infinity and its restart from P) and sums of a G2 point and a small-order one; the same
sets as 130 one-set jobs (per-set statuses) and as 13 jobs of ten (per-job statuses), and the edge
shapes n = 1 and n = 64.  Statuses must be identical, not close."""
import os

import numpy as np
import pytest

from lodestar_amd.engine import SetInput
from test_gpu_parity import H2, R, case_jobs, interop_sk

pytestmark = pytest.mark.gpu

N_SETS = 130


def _engine_with(env):
    from lodestar_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(0)  # the engine reads its form switches once, here
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def forms():
    """the lone-lane form for every batch size, and the 8-lane form for every batch size"""
    lone = _engine_with({"LB_SUBGROUP_G8_MAX": "0", "LB_ROW_FE": "0"})
    g8 = _engine_with({"LB_SUBGROUP_G8_MAX": str(1 << 31), "LB_ROW_FE": "0"})
    yield {"lone": lone, "g8": g8}
    lone.close()
    g8.close()


def _oracle_sig_status(sig):
    """the oracle's Signature.fromBytes(sig, validate=true): an error name, "inf" or "ok" """
    import oracle.bls_oracle as o
    try:
        return "inf" if o.signature_from_bytes(sig, True) is None else "ok"
    except o.BlsError as e:
        return str(e)


@pytest.fixture(scope="module")
def batch(forms):
    """130 sets and, per set, the oracle's verdict on its signature; every set's key and message are
    right for its signature where the signature is a valid one, so a set is True exactly when the
    oracle decodes its signature into G2"""
    import oracle.bls_oracle as o
    e = forms["g8"]
    rng = np.random.default_rng(28)
    pool = [interop_sk(i) for i in range(16)]
    _, pk96 = e.sk_to_pk(pool)
    msgs = rng.integers(0, 256, size=(N_SETS, 32), dtype=np.uint8)
    idx = rng.integers(0, 16, size=N_SETS)
    sigs = e.sign([pool[j] % R for j in idx], msgs)
    sets = [SetInput([pk96[idx[i]].tobytes()], msgs[i].tobytes(), sigs[i].tobytes()) for i in range(N_SETS)]
    cases, jobs = case_jobs()
    golden = {c["name"]: j for c, j in zip(cases, jobs)}
    special = {}
    special[5] = golden["infinity_signature_single"][0].signature
    special[17] = golden["invalid_size_32_zero"][0].signature
    special[40] = golden["not_on_curve"][0].signature
    special[51] = golden["bad_encoding_x_ge_p"][0].signature
    special[63] = golden["not_in_group"][0].signature
    mapped = lambda s: o.iso_map(o.map_to_curve_sswu(o.hash_to_field_fp2(bytes([s]) * 32, 2, o.DST_POP)[0]))  # noqa: E731
    for k, pos in enumerate((0, 31, 64, 65, 100, 127)):          # curve points outside G2
        special[pos] = o.g2_compress(mapped(k))
    small = []
    q = mapped(0x20)
    for ell in (13, 23):
        Q = o.g2_mul(q, H2 * o.R // (ell * ell))
        if Q is not None and o.g2_mul(Q, ell) is not None:
            Q = o.g2_mul(Q, ell)
        assert Q is not None and o.g2_mul(Q, ell) is None
        small += [Q, o.g2_neg(Q), o.g2_mul(Q, 2), o.g2_mul(Q, 5)]
    for Q, pos in zip(small, (1, 32, 62, 66, 96, 126, 128, 129)):  # both waves, and the 2-lane tail
        special[pos] = o.g2_compress(Q)
    g = o.g2_clear_cofactor(mapped(0x21))
    special[70] = o.g2_compress(o.g2_add(g, small[0]))
    special[71] = o.g2_compress(o.g2_add(g, small[4]))
    for pos, sig in special.items():
        sets[pos] = SetInput(sets[pos].pubkeys, sets[pos].signing_root, sig)
    sets[90] = golden["single_valid_0"][0]                         # a valid set the oracle itself verified
    status = [_oracle_sig_status(s.signature) for s in sets]
    assert {"ok", "inf", "BLST_INVALID_SIZE", "BLST_POINT_NOT_ON_CURVE", "BLST_BAD_ENCODING",
            "BLST_POINT_NOT_IN_GROUP"} == set(status)
    assert status.count("BLST_POINT_NOT_IN_GROUP") == 17 and status.count("ok") == N_SETS - 21
    return sets, status


def _expected(job_status):
    """a job's result from its sets' oracle statuses: the first signature error in set order, else
    False for an infinity signature, else True"""
    for s in job_status:
        if s not in ("ok", "inf"):
            return s
    return "inf" not in job_status


def _named(engine_codes):
    from lodestar_amd import _native as N
    return [N.error_name(-c) if c < 0 else bool(c) for c in engine_codes]


@pytest.mark.parametrize("n,per_job", [(N_SETS, 1), (N_SETS, 10), (64, 1), (1, 1)])
def test_lone_lane_statuses_equal_g8_and_oracle(forms, batch, n, per_job):
    sets, status = batch
    jobs = [sets[i:i + per_job] for i in range(0, n, per_job)]
    exp = [_expected(status[i:i + per_job]) for i in range(0, n, per_job)]
    lone = _named(forms["lone"].verify_jobs(jobs))
    g8 = _named(forms["g8"].verify_jobs(jobs))
    assert lone == g8
    assert lone == exp


def test_one_set_each_kind(forms, batch):
    """n = 1 again: a point of order 13 (set 1), a valid signature (set 2), the infinity signature (set 5)"""
    sets, status = batch
    assert [status[i] for i in (1, 2, 5)] == ["BLST_POINT_NOT_IN_GROUP", "ok", "inf"]
    for form in ("lone", "g8"):
        assert [_named(forms[form].verify_jobs([[sets[i]]]))[0] for i in (1, 2, 5)] == ["BLST_POINT_NOT_IN_GROUP", True, False]
