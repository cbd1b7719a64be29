"""k_miller_lane on its limb-resident loop (lb_pairing.h miller_lane28) against the 8-lane form
k_miller_g8, whose arithmetic this change leaves alone.  Engines are pinned to the per-root form by
the engine's own switches: LB_ALONE = 0 and LB_ROW_FE = 0 first, because an engine that finds the
device to itself sends up to 256 roots to the row form (k_miller_row) before it looks at any other
switch, and with three engines in one process that depends on timing; then LB_MILLER_FORM,
LB_MILLER_WAVE_MAX = 0 so that not even a one-root batch goes to the wave form, and
LB_MILLER_LDS3_MAX for k_miller_lane<3> or <2>.  profiles/miller_limb_kernel_trace.txt records the
Miller kernels this file launches: two lane dispatches per form and batch (verify and partial), no
row or wave form.  Batches of 1, 64 and 65 distinct roots, one set each: a single live lane, a
full wave, and a second workgroup with one lane.  The 65-root batch holds a root whose only set
carries a malformed signature, so its P_u is the point at infinity and the leaf is written as
f = 1; every other set is valid, so the root check of verify passes only if that leaf and the
other 64 are right.  With fixed blinding scalars the verdicts must be the planted ones and the
576-byte root partial byte-identical to the 8-lane form's, not close."""
import os

import numpy as np
import pytest

from lodestar_amd.engine import SetInput, pack_jobs
from test_gpu_parity import R, interop_sk

pytestmark = pytest.mark.gpu

BIG = str(1 << 31)
PIN = {"LB_ALONE": "0", "LB_ROW_FE": "0", "LB_MILLER_WAVE_MAX": "0"}  # never the row or the wave form
FORMS = {
    "lane3": {**PIN, "LB_MILLER_FORM": "lane", "LB_MILLER_LDS3_MAX": BIG},
    "lane2": {**PIN, "LB_MILLER_FORM": "lane", "LB_MILLER_LDS3_MAX": "0"},
    "g8": {**PIN, "LB_MILLER_FORM": "g8", "LB_MILLER_LDS3_MAX": BIG},
}
MALFORMED = 7  # position in the 65-root batch


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
def engines():
    es = {name: _engine_with(env) for name, env in FORMS.items()}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def sets(engines):
    """n -> n sets with n distinct signing roots, one set each: the valid sets 0 .. n - 1, and for
    n = 65 the malformed signature planted among them"""
    e = engines["g8"]
    rng = np.random.default_rng(2812)
    pool = [interop_sk(i) for i in range(8)]
    _, pk96 = e.sk_to_pk(pool)
    msgs = rng.integers(0, 256, size=(65, 32), dtype=np.uint8)
    assert len({m.tobytes() for m in msgs}) == 65
    idx = rng.integers(0, 8, size=65)
    sigs = e.sign([pool[j] % R for j in idx], msgs)
    valid = [SetInput([pk96[idx[i]].tobytes()], msgs[i].tobytes(), sigs[i].tobytes()) for i in range(65)]
    planted = list(valid)
    planted[MALFORMED] = SetInput(valid[MALFORMED].pubkeys, valid[MALFORMED].signing_root, bytes(32))
    return {1: valid[:1], 64: valid[:64], 65: planted}


def _run(engine, batch_sets):
    from lodestar_amd import _native as N
    sc = np.random.default_rng(5).integers(1, 1 << 63, size=len(batch_sets), dtype=np.uint64)
    b = engine.upload(pack_jobs([[s] for s in batch_sets]))
    try:
        codes = b.verify(scalars=sc).tolist()
        raw, st = b.partial(scalars=sc)
    finally:
        b.free()
    return [N.error_name(-c) if c < 0 else bool(c) for c in codes], bytes(raw), st.tolist()


_G8 = {}


def _g8(engines, sets, n):
    if n not in _G8:
        _G8[n] = _run(engines["g8"], sets[n])
    return _G8[n]


@pytest.mark.parametrize("form", ["lane3", "lane2"])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_lane_partial_byte_identical_to_g8(engines, sets, n, form):
    exp = [True] * n
    if n == 65:
        exp[MALFORMED] = "BLST_INVALID_SIZE"
    ref_verdicts, ref_raw, ref_st = _g8(engines, sets, n)
    assert ref_verdicts == exp
    verdicts, raw, st = _run(engines[form], sets[n])
    assert verdicts == exp
    assert st == ref_st
    assert len(raw) == 576 and raw == ref_raw
