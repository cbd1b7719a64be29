"""The signatures' subgroup check once per batch (k_subgroup_mix, k_subgroup_affine,
k_sig_subgroup_g8 over the mixed points, k_subgroup_flag, and the rerun by the per-set kernel) on the device.

Engines are pinned so that small batches take the bucket MSM and the lone forms (LB_SMALL_S_MAX=0,
LB_ALONE=0, LB_ROW_FE=0), once with LB_MSM_G8=0 and once with 1, each with LB_SUBGROUP_BATCH=1 and, as the
reference, 0 (the pipeline as it was).  The engine draws the blinding words and the tests' bits itself, so
every call is a fresh draw; every adversarial case runs 8 calls and each must reject (the bound is 2^-64 per
call).  Sizes: 65 and 130 sets, two waves and a partial wave of the per-set kernels.

The non-subgroup signatures are the points of tests/golden/subgroup28_points.txt (order 13, order 23, curve
points of large cofactor order, a G2 point plus a small-order one), compressed here; that the reference
engine answers BLST_POINT_NOT_IN_GROUP for them (and not a decode error) checks the compression."""
import os

import numpy as np
import pytest

import test_forgeries_gpu as FG
from lodestar_amd import _native as N
from lodestar_amd.engine import SetInput, pack_jobs
from test_gpu_parity import make_batch, make_shared_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
PINS = {"LB_SMALL_S_MAX": "0", "LB_ALONE": "0", "LB_ROW_FE": "0"}
NOT_IN_GROUP = -N.LB_POINT_NOT_IN_GROUP
CALLS = 8
SIZES = [65, 130]
G8 = ["0", "1"]


def _engine_with(env):
    from lodestar_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(0)  # the engine reads its switches once, here
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    """(LB_MSM_G8, LB_SUBGROUP_BATCH) -> engine"""
    es = {(g8, sb): _engine_with({**PINS, "LB_MSM_G8": g8, "LB_SUBGROUP_BATCH": sb}) for g8 in G8 for sb in ("0", "1")}
    yield es
    for e in es.values():
        e.close()


def compress_g2(x0, x1, y0, y1):
    """ZCash compressed form of an affine point of E'(Fp2): x.c1 || x.c0, flags in the top bits"""
    n0, n1 = (P - y0) % P, (P - y1) % P
    largest = y1 > n1 if y1 != n1 else y0 > n0
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if largest else 0)
    return bytes(b)


def neg_sig(sig):
    return bytes([sig[0] ^ 0x20]) + sig[1:]


@pytest.fixture(scope="module")
def outside():
    """kind -> compressed signatures outside G2 (kinds: ord13, ord23, curve, mixed)"""
    out = {}
    with open(os.path.join(ROOT, "tests", "golden", "subgroup28_points.txt")) as f:
        for line in f:
            kind, in_group, *h = line.split()
            if in_group == "0":
                out.setdefault(kind, []).append(compress_g2(*(int(v, 16) for v in h)))
    assert set(out) == {"ord13", "ord23", "curve", "mixed"}
    return out


_VALID = {}


def valid_jobs(engine, n):
    """n valid single-set jobs over distinct roots, signed once per module on the session engine"""
    if n not in _VALID:
        _VALID[n] = make_batch(engine, n, seed=100 + n)
    return [list(j) for j in _VALID[n]]


def with_sigs(jobs, sigs):
    """jobs with the signature of job p's first set replaced, for every p of sigs"""
    jobs = [list(j) for j in jobs]
    for p, sig in sigs.items():
        s = jobs[p][0]
        jobs[p][0] = SetInput(s.pubkeys, s.signing_root, sig)
    return jobs


def counted(e, call):
    """the call's result and how far it moved (runs, fallbacks) of lb_subgroup_batch_runs"""
    r0, f0 = e.subgroup_batch_runs()
    out = call()
    r1, f1 = e.subgroup_batch_runs()
    return out, r1 - r0, f1 - f0


@pytest.mark.parametrize("g8", G8)
@pytest.mark.parametrize("n", SIZES)
def test_all_valid_one_test_per_batch_no_fallback(engine, engines, n, g8):
    jobs = valid_jobs(engine, n)
    e = engines[(g8, "1")]
    for _ in range(2):
        codes, runs, fb = counted(e, lambda: e.verify_jobs(jobs))
        assert codes == [1] * n
        assert (runs, fb) == (1, 0)
    codes, runs, fb = counted(engines[(g8, "0")], lambda: engines[(g8, "0")].verify_jobs(jobs))
    assert codes == [1] * n and (runs, fb) == (0, 0)  # switched off: the counter stands still


@pytest.mark.parametrize("g8", G8)
@pytest.mark.parametrize("n", SIZES)
def test_one_signature_outside_the_group(engine, engines, outside, n, g8):
    """exactly that job is BLST_POINT_NOT_IN_GROUP, the others as without the batch test, one fallback per call"""
    e, ref = engines[(g8, "1")], engines[(g8, "0")]
    for k, (kind, pos) in enumerate([("ord13", 0), ("ord23", 63), ("curve", 64), ("mixed", n - 1)]):
        jobs = with_sigs(valid_jobs(engine, n), {pos: outside[kind][k % len(outside[kind])]})
        want = ref.verify_jobs(jobs)
        assert want == [NOT_IN_GROUP if j == pos else 1 for j in range(n)], kind
        for _ in range(CALLS):
            codes, runs, fb = counted(e, lambda: e.verify_jobs(jobs))
            assert codes == want, kind
            assert (runs, fb) == (1, 1), kind  # the rerun takes the per-set kernel: one run of the batch test


@pytest.mark.parametrize("g8", G8)
@pytest.mark.parametrize("n", SIZES)
def test_same_point_twice_and_point_with_its_negative(engine, engines, outside, n, g8):
    e, ref = engines[(g8, "1")], engines[(g8, "0")]
    t13, big = outside["ord13"][0], outside["curve"][1]
    for sigs in ({3: t13, 70 % n: t13}, {3: t13, 64: neg_sig(t13)}, {1: big, 2: big}, {n - 2: big, n - 1: neg_sig(big)}):
        jobs = with_sigs(valid_jobs(engine, n), sigs)
        want = ref.verify_jobs(jobs)
        assert want == [NOT_IN_GROUP if j in sigs else 1 for j in range(n)]
        for _ in range(CALLS):
            codes, runs, fb = counted(e, lambda: e.verify_jobs(jobs))
            assert codes == want
            assert (runs, fb) == (1, 1)


@pytest.mark.parametrize("g8", G8)
def test_cancelling_pair_and_forgeries_as_without_the_batch_test(engine, engines, g8):
    """tests/golden/cancel_pair.json (shapes A, F) and forgeries.json (B, B_job, C, G): signatures of G2 whose
    errors cancel under equal weights.  The batch test must not fire, and the codes are the per-set pipeline's."""
    S = FG.shapes(engine)
    e, ref = engines[(g8, "1")], engines[(g8, "0")]
    for name in ("A", "B", "B_job", "C", "F", "G"):
        sh = S[name]
        want = ref.verify_jobs_packed(sh.packed)
        assert want == sh.expected, name
        for _ in range(CALLS):
            codes, runs, fb = counted(e, lambda: e.verify_jobs_packed(sh.packed))
            assert codes == want, name
            assert (runs, fb) == (1, 0), name


@pytest.mark.parametrize("g8", G8)
@pytest.mark.parametrize("shape", ["c3", "aggregate"])
def test_equal_codes_and_partials_with_and_without(engine, engines, outside, shape, g8):
    """c3-shaped (many sets on few roots, one wrong-message set) and aggregate-shaped (four keys per set)
    small batches: equal codes; byte-identical 576-byte partials under the same blinding words; under the
    engine's own words the partial call takes the batch test too and its statuses are equal"""
    n = 130
    if shape == "c3":
        jobs = make_shared_batch(engine, n, 4, seed=7, invalid={77})
        want = [0 if j == 77 else 1 for j in range(n)]
    else:
        jobs = make_batch(engine, n, agg_k=4, seed=9)
        want = [1] * n
    e, ref = engines[(g8, "1")], engines[(g8, "0")]
    packed = pack_jobs(jobs)
    words = np.random.default_rng(n).integers(1, 1 << 63, size=n, dtype=np.uint64)
    codes, runs, fb = counted(e, lambda: e.verify_jobs_packed(packed))
    assert codes == ref.verify_jobs_packed(packed) == want
    assert (runs, fb) == (1, 0)  # a signature over another message is still a point of G2
    be, br = e.upload(packed), ref.upload(packed)
    try:
        (pe, se), runs, fb = counted(e, lambda: be.partial(scalars=words))
        pr, sr = br.partial(scalars=words)
        assert pe == pr and len(pe) == 576
        assert se.tolist() == sr.tolist() == [1] * n
        assert (runs, fb) == (0, 0)
        (pe, se), runs, fb = counted(e, be.partial)
        assert se.tolist() == [1] * n and (runs, fb) == (1, 0)
        assert be.search_after_partial(fallback=False).tolist() == want
        assert e.product_is_one([pe]) == (shape == "aggregate")
    finally:
        be.free()
        br.free()
    # ... and with a signature outside the group the partial call falls back and reports it per job
    bad = pack_jobs(with_sigs(jobs, {5: outside["ord23"][1]}))
    be, br = e.upload(bad), ref.upload(bad)
    try:
        (pe, se), runs, fb = counted(e, be.partial)
        assert se.tolist() == br.partial()[1].tolist() == [NOT_IN_GROUP if j == 5 else 1 for j in range(n)]
        assert (runs, fb) == (1, 1)
    finally:
        be.free()
        br.free()


@pytest.mark.parametrize("g8", G8)
def test_caller_given_scalars_take_the_per_set_kernel(engine, engines, outside, g8):
    e = engines[(g8, "1")]
    n = 65
    words = np.random.default_rng(3).integers(1, 1 << 63, size=n, dtype=np.uint64)
    jobs = valid_jobs(engine, n)
    codes, runs, fb = counted(e, lambda: e.verify_jobs(jobs, scalars=words))
    assert codes == [1] * n and (runs, fb) == (0, 0)
    jobs = with_sigs(jobs, {64: outside["ord13"][2]})
    codes, runs, fb = counted(e, lambda: e.verify_jobs(jobs, scalars=words))
    assert codes == [1] * 64 + [NOT_IN_GROUP] and (runs, fb) == (0, 0)


@pytest.mark.parametrize("g8", G8)
def test_dead_job_with_an_untested_signature(engine, engines, outside, g8):
    """Only live sets enter the MSM.  A job that another error kills may hold a signature outside the group
    whose verdict the per-set pipeline reports first (set order among the signature errors; before an
    infinite pubkey): such a batch falls back.  Where the other error comes first, it does not."""
    e, ref = engines[(g8, "1")], engines[(g8, "0")]
    v = valid_jobs(engine, 65)
    t = outside["curve"][2]
    bad_enc = bytes([v[1][0].signature[0] & 0x7F]) + v[1][0].signature[1:]
    s0, s1 = v[0][0], v[1][0]
    first = [[SetInput(s0.pubkeys, s0.signing_root, t), SetInput(s1.pubkeys, s1.signing_root, bad_enc)]] + v[2:]
    codes, runs, fb = counted(e, lambda: e.verify_jobs(first))
    assert codes == ref.verify_jobs(first) == [NOT_IN_GROUP] + [1] * 63
    assert (runs, fb) == (1, 1)
    second = [[SetInput(s1.pubkeys, s1.signing_root, bad_enc), SetInput(s0.pubkeys, s0.signing_root, t)]] + v[2:]
    codes, runs, fb = counted(e, lambda: e.verify_jobs(second))
    assert codes == ref.verify_jobs(second) == [-N.LB_BAD_ENCODING] + [1] * 63
    assert (runs, fb) == (1, 0)
