"""Which kernel form each stage of a batch verification runs (lodestar_amd/csrc/lb_pipeline_plan.h) on the
CPU, through build/lb_pipeline_harness.so.

1. The header against a model of the selection as it stood inside lb_engine.hip at commit 0b98081
   (run_pipeline, per_root_chain, msm_reduce, search_round, search_invalid, batch_fill, verify_locked,
   lb_fp12_product_is_one), transcribed below condition by condition with the engine's own names; every
   plan field on every point of a grid: every threshold a function reads at 0, 1, T - 1, T, T + 1 (T its
   default) and 2^31 where a test pins it there, both values of every boolean and pin, every "alone" sample
   on its own, n and nuh <= n from N_GRID.
2. The environment table against the values the getenv lines of lb_engine_create_ex gave, written out.
3. The pinned environments of the GPU tests: the plan at their batch sizes names the kernel their
   docstrings say they exercise."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 31
N_GRID = [1, 2, 7, 8, 9, 64, 65, 256, 257, 2048, 2049, 4096, 4097, 32768, 32769]

# the knobs, in the order of the header's table: variable -> (engine field at 0b98081, default)
VARS = {
    "LB_MILLER_WAVE_MAX": ("miller_wave_max", 2048), "LB_ROW_MAX": ("row_max", 256), "LB_ROW_FE": ("row_fe", 1),
    "LB_MILLER_LDS3_MAX": ("miller_lds3_max", 32768), "LB_MILLER_FORM": ("miller_form", 0),
    "LB_HASH_G8_MAX": ("hash_g8_max", 2048), "LB_HASH_ROW_MAX": ("hash_row_max", 256),
    "LB_DEC_ROW_MAX": ("dec_row_max", 4096), "LB_SUBGROUP_G8_MAX": ("subgroup_g8_max", 4096),
    "LB_SMALL_S_MAX": ("small_s_max", 32768), "LB_SMALL_S_G8_MAX": ("small_s_g8_max", 2048),
    "LB_SEARCH_SMALL_MAX": ("search_small_max", 32768), "LB_SMSM_FORM": ("smsm_form", 0), "LB_MSM_G8": ("msm_g8", 1),
    "LB_ALONE": ("alone_force", -1),
}
FIELDS = [f for f, _ in VARS.values()]
DEFAULTS = {f: d for f, d in VARS.values()}
COUNTS = {"miller_wave_max", "row_max", "miller_lds3_max", "hash_g8_max", "hash_row_max", "dec_row_max",
          "subgroup_g8_max", "small_s_max", "small_s_g8_max", "search_small_max"}
# thresholds a test pins at 2^31 (test_gpu_parity, test_miller28_gpu, test_subgroup28_gpu, test_forgeries_gpu)
PINNED_BIG = {"miller_wave_max", "miller_lds3_max", "hash_g8_max", "subgroup_g8_max", "small_s_max", "small_s_g8_max",
              "search_small_max"}

# the forms, numbered as the header's enums
FE_ROW, FE_WAVE = 0, 1
GSUM_WAVE, GSUM_CHUNKS = 0, 1
PK_ON_S3, PK_ON_S2 = 0, 1
PKC_NONE, PKC_INDEXED, PKC_BYTES = 0, 1, 2
PKB_ONE_PASS, PKB_SPLIT, PKB_SPLIT_ROWP, PKB_ROUTE = 0, 1, 2, 3
DEC_ROW, DEC_LANE = 0, 1
SUBGROUP_W4, SUBGROUP_G8, SUBGROUP_LANE = 0, 1, 2
GROUP_ONE_SET, GROUP_DEVICE_ORDER, GROUP_HOST_ORDER = 0, 1, 2
SSUM_PAR_W4, SSUM_UNBLINDED, SSUM_TERMS_G8, SSUM_TERMS_LANE, SSUM_BUCKET_MSM = 0, 1, 2, 3, 4
HMAP_ROW, HMAP_LANE = 0, 1
HFIN_ROW, HFIN_G8, HFIN_LANE = 0, 1, 2
MILLER_ROW, MILLER_WAVE, MILLER_LANE3, MILLER_LANE2, MILLER_G8 = 0, 1, 2, 3, 4
MSMB_G8, MSMB_LANE = 0, 1
MSMR_WINDOW_HORNER, MSMR_REDUCE = 0, 1
SRCH_NO_SUMS, SRCH_TERMS, SRCH_BUCKET_MSM = 0, 1, 2
STERMS_ROOT_SUMS, STERMS_LANE, STERMS_G8 = 0, 1, 2
BATCH_FIELDS = ["alone", "row", "row_small", "gsum", "pk_on", "pk_chunks", "pk_blind", "decode", "subgroup", "group",
                "ssum", "fe"]

U8P, U32P, U64P, I64P = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_pipeline_harness
    lib = ctypes.CDLL(build_pipeline_harness(verbose=False))
    lib.c_pipe_knob_count.restype = ctypes.c_uint32
    lib.c_pipe_knob_name.restype = ctypes.c_char_p
    lib.c_pipe_knob_name.argtypes = [ctypes.c_uint32]
    assert [lib.c_pipe_knob_name(i).decode() for i in range(lib.c_pipe_knob_count())] == list(VARS)
    return lib


class K:
    """one setting of the knobs: the defaults, with some replaced"""

    def __init__(self, **kw):
        self.__dict__.update(DEFAULTS)
        assert set(kw) <= set(DEFAULTS)
        self.__dict__.update(kw)

    def raw(self):
        return np.array([getattr(self, f) for f in FIELDS], dtype=np.int64)


def call(fn, k, m, ins, width):
    out = np.zeros((m, width), dtype=np.uint8)
    ptr = {np.dtype(np.uint8): U8P, np.dtype(np.uint32): U32P, np.dtype(np.uint64): U64P}
    raw = k.raw()
    ins = [np.ascontiguousarray(a) for a in ins]
    fn(raw.ctypes.data_as(I64P), ctypes.c_uint32(m), *[a.ctypes.data_as(ptr[a.dtype]) for a in ins],
       out.ctypes.data_as(U8P))
    return out


def values(field):
    t = DEFAULTS[field]
    return sorted({0, 1, t - 1, t, t + 1} | ({BIG} if field in PINNED_BIG else set()))


def knob_grid(*fields, **fixed):
    """every combination of the counts' threshold values and of the booleans' and pins' values"""
    axes = [values(f) if f in COUNTS else [0, 1, 2] if f.endswith("_form") else [0, 1] for f in fields]
    for combo in itertools.product(*axes):
        yield K(**dict(zip(fields, combo)), **fixed)


def columns(*axes):
    """the cross product of the axes, one int64 column per axis"""
    g = np.meshgrid(*[np.asarray(a, dtype=np.int64) for a in axes], indexing="ij")
    return [x.ravel() for x in g]


def pick(*pairs):
    """nested a ? x : b ? y : ... : z over arrays: pick(c0, v0, c1, v1, ..., default)"""
    out = np.broadcast_to(np.asarray(pairs[-1], dtype=np.int64), np.shape(pairs[0])).copy()
    for c, v in reversed(list(zip(pairs[0:-1:2], pairs[1:-1:2]))):
        out = np.where(c, v, out)
    return out


def same(got, want, names, k, cols):
    for j, name in enumerate(names):
        bad = np.nonzero(got[:, j] != want[j])[0]
        assert not len(bad), (name, "header %d, model %d" % (got[bad[0], j], want[j][bad[0]]), vars(k),
                              [int(c[bad[0]]) for c in cols])


# ---------------------------------------------------------------------------- the model (commit 0b98081)
def model_batch(e, n, nc, n_comb, indexed, routed_here, scalars, unblinded, root_shuffle, alone):
    """run_pipeline: e->alone = device_alone(e) at its start; b->n_chunks, b->n_comb, b->indexed,
    b->route_eng == e; `scalars` non-null; e->root_shuffle"""
    row = alone & bool(e.row_fe)                      # const bool row = e->alone && e->row_fe;
    row_small = row & (n <= e.row_max)                # const bool row_small = row && n <= e->row_max;
    one_unblinded = (n == 1) & ~scalars & unblinded   # n == 1 && !scalars && unblinded
    gsum = pick(alone, GSUM_WAVE, GSUM_CHUNKS)        # e->gchunk = e->alone ? LB_GROUP_CHUNK_WAVE : ...; if (e->alone) k_gsum_wave
    on_s3 = n <= e.small_s_max                        # const hipStream_t s3 = n <= e->small_s_max ? s3_ : s2;
    pk_chunks = pick((nc > 0) & indexed, PKC_INDEXED, nc > 0, PKC_BYTES, PKC_NONE)  # if (nc && b->indexed) .. else if (nc)
    pk_split = on_s3                                  # const bool pk_split = s3 != s2;
    pk_rowp = pk_split & row_small                    # const bool pk_rowp = pk_split && row_small;
    sb_par = pk_split & ~one_unblinded & row_small & (n <= e.small_s_max) & (n <= e.small_s_g8_max)
    route = indexed & (n_comb > 0) & routed_here & ~pk_rowp
    # if (route) {mode 1, comb, mode 2 over the rest}; else modes m0 .. m1 = pk_split ? 1, 2 : 0, 0, mode 2 by rows if pk_rowp
    pk_blind = pick(route, PKB_ROUTE, ~pk_split, PKB_ONE_PASS, pk_rowp, PKB_SPLIT_ROWP, PKB_SPLIT)
    decode = pick(row & (n <= e.dec_row_max), DEC_ROW, DEC_LANE)
    subgroup = pick(row_small, SUBGROUP_W4, n <= e.subgroup_g8_max, SUBGROUP_G8, SUBGROUP_LANE)
    group = pick(n == 1, GROUP_ONE_SET, root_shuffle, GROUP_DEVICE_ORDER, GROUP_HOST_ORDER)
    ssum = pick(sb_par, SSUM_PAR_W4, one_unblinded, SSUM_UNBLINDED,
                (n <= e.small_s_max) & (n <= e.small_s_g8_max), SSUM_TERMS_G8, n <= e.small_s_max, SSUM_TERMS_LANE,
                SSUM_BUCKET_MSM)
    fe = pick(row, FE_ROW, FE_WAVE)                   # if (row) k_ml_S_row; (e->alone && e->row_fe) ? k_root_check_row : ...
    return [alone, row, row_small, gsum, pick(on_s3, PK_ON_S3, PK_ON_S2), pk_chunks, pk_blind, decode, subgroup, group,
            ssum, fe]


def model_roots(e, nuh, lo, alone, alone_hash, alone_miller):
    """run_pipeline after the grouping (alone_hash: the device_alone of ST_HASH_FIN) and per_root_chain
    (alone_miller: the device_alone of ST_MILLER)"""
    row = alone & bool(e.row_fe)
    row_hash = row & (nuh <= e.hash_row_max)          # const bool row_hash = row && nuh <= e->hash_row_max;
    hmap = pick(row_hash, HMAP_ROW, HMAP_LANE)
    a = (e.miller_form == 0) & alone_hash             # const bool alone = e->miller_form == 0 && device_alone(e);
    fin = pick(row_hash, HFIN_ROW, (nuh <= e.hash_g8_max) | a, HFIN_G8, HFIN_LANE)
    row_roots = row & (nuh <= e.row_max)              # const bool row_roots = row && nuh <= e->row_max;
    shared = (e.miller_form == 1) | ((e.miller_form == 0) & ~alone_miller)
    miller = pick(row_roots, MILLER_ROW, nuh <= e.miller_wave_max, MILLER_WAVE,
                  shared & (nuh <= e.miller_lds3_max), MILLER_LANE3, shared, MILLER_LANE2, MILLER_G8)
    tree = pick(row & (lo <= e.row_max), FE_ROW, FE_WAVE)  # if (row && lo <= e->row_max) k_tree_up_row
    return [hmap, fin, miller, tree]


def model_msm(e, entries, chunk, nb, alone_now):
    """msm_reduce: if (e->msm_g8) {(entries >= 4 * chunk * nb && device_alone(e)) ? buckets_g8 : buckets; window, horner}
    else {buckets; reduce}"""
    g8 = bool(e.msm_g8)
    return [pick(g8 & (entries >= 4 * chunk * nb) & alone_now, MSMB_G8, MSMB_LANE),
            pick(np.full(entries.shape, g8), MSMR_WINDOW_HORNER, MSMR_REDUCE)]


def model_search_round(e, cm, T, rs_path, alone_now):
    """search_round: if (cm && T && (rs_path || T <= e->search_small_max)) {rs_path ? k_rsm_terms : smsm_form == 1 ||
    (smsm_form == 0 && !device_alone(e)) ? lane : g8} else if (cm) {bucket MSM}"""
    terms_round = (cm > 0) & (T > 0) & (rs_path | (T <= e.search_small_max))
    sums = pick(terms_round, SRCH_TERMS, cm > 0, SRCH_BUCKET_MSM, SRCH_NO_SUMS)
    lane = (e.smsm_form == 1) | ((e.smsm_form == 0) & ~alone_now)
    return sums, pick(rs_path, STERMS_ROOT_SUMS, lane, STERMS_LANE, STERMS_G8), terms_round


def model_search_start(e, n, nu, search_blk, search_rootsum):
    """search_invalid"""
    r1_plain = search_blk & (nu > 1) & (n > e.search_small_max)
    return [r1_plain, ~r1_plain & search_rootsum & (nu > 1) & (n > e.search_small_max)]


# ---------------------------------------------------------------------------- 1. header against model
def test_batch_plan_equals_the_parents_selection(L):
    # shapes: n x chunks x (indexed, n_comb, routed) x scalars x unblinded x root_shuffle x alone
    cols = columns(N_GRID, [0, 5], [0, 1], [0, 3], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1])
    n, nc, indexed, n_comb, routed, scalars, unblinded, shuffle, alone = cols
    flags = (indexed | routed << 1 | scalars << 2 | unblinded << 3 | shuffle << 4 | alone << 5).astype(np.uint8)
    ins = [n.astype(np.uint32), nc.astype(np.uint32), n_comb.astype(np.uint32), flags]
    b = [c.astype(bool) for c in (indexed, routed, scalars, unblinded, shuffle, alone)]
    points = 0
    for k in knob_grid("row_fe", "row_max", "small_s_max", "small_s_g8_max", "dec_row_max", "subgroup_g8_max"):
        got = call(L.c_pipe_batch, k, len(n), ins, 12)
        want = model_batch(k, n, nc, n_comb, b[0], b[1], b[2], b[3], b[4], b[5])
        same(got, want, BATCH_FIELDS, k, cols)
        points += len(n)
    assert points == 2 * 5 * 6 * 6 * 5 * 6 * 15 * 2 ** 8


def test_per_root_plans_equal_the_parents_selection(L):
    pairs = [(a, b) for a in N_GRID for b in N_GRID if b <= a]
    idx, lo, alone, alone_hash, alone_miller = columns(range(len(pairs)), [1, 64, 256, 257, 16384], [0, 1], [0, 1], [0, 1])
    n, nuh = np.array(pairs, dtype=np.int64)[idx].T
    cols = [n, nuh, lo, alone, alone_hash, alone_miller]
    flags = (alone | alone_hash << 1 | alone_miller << 2).astype(np.uint8)
    ins = [n.astype(np.uint32), nuh.astype(np.uint32), lo.astype(np.uint32), flags]
    a, ah, am = (c.astype(bool) for c in (alone, alone_hash, alone_miller))
    names = ["hash_map", "hash_fin", "miller", "tree"]
    # the hash plan's knobs, then the Miller loop's and the tree's
    for k in itertools.chain(knob_grid("row_fe", "hash_row_max", "hash_g8_max", "miller_form"),
                             knob_grid("row_fe", "row_max", "miller_wave_max", "miller_lds3_max", "miller_form")):
        same(call(L.c_pipe_roots, k, len(n), ins, 4), model_roots(k, nuh, lo, a, ah, am), names, k, cols)


def test_bucket_reduction_plan_equals_the_parents_selection(L):
    # (chunk, buckets): the batch MSM's and a search round's; entries around 4 * chunk * nb, and 2^33
    for chunk, nb in ((32, 2048), (8, 109 * 2 * 256), (1, 1), (64, 1 << 20)):
        t = 4 * chunk * nb
        entries, alone_now = columns([0, 1, t - 1, t, t + 1, 1 << 33], [0, 1])
        cols = [entries, alone_now]
        ins = [entries.astype(np.uint64), np.full(len(entries), chunk, np.uint32), np.full(len(entries), nb, np.uint32),
               alone_now.astype(np.uint8)]
        for k in knob_grid("msm_g8"):
            want = model_msm(k, entries, chunk, nb, alone_now.astype(bool))
            same(call(L.c_pipe_msm, k, len(entries), ins, 2), want, ["buckets", "reduce"], k, cols)


def test_search_plans_equal_the_parents_selection(L):
    cols = columns([0, 1, 109], [0] + N_GRID + [BIG], [0, 1], [0, 1])
    cm, T, rs_path, alone_now = cols
    ins = [cm.astype(np.uint32), T.astype(np.uint32), (rs_path | alone_now << 1).astype(np.uint8)]
    for k in knob_grid("search_small_max", "smsm_form"):
        got = call(L.c_pipe_search_round, k, len(cm), ins, 2)
        sums, terms, terms_round = model_search_round(k, cm, T, rs_path.astype(bool), alone_now.astype(bool))
        same(got[:, :1], [sums], ["sums"], k, cols)
        same(got[terms_round, 1:], [terms[terms_round]], ["terms"], k, [c[terms_round] for c in cols])  # launched only then
    pairs = [(a, b) for a in N_GRID for b in N_GRID if b <= a]
    idx, blk, rootsum = columns(range(len(pairs)), [0, 1], [0, 1])
    n, nu = np.array(pairs, dtype=np.int64)[idx].T
    ins = [n.astype(np.uint32), nu.astype(np.uint32), (blk | rootsum << 1).astype(np.uint8)]
    for k in knob_grid("search_small_max"):
        want = model_search_start(k, n, nu, blk.astype(bool), rootsum.astype(bool))
        same(call(L.c_pipe_search_start, k, len(n), ins, 2), want, ["r1_plain", "root_sums"], k, [n, nu, blk, rootsum])


def test_chunk_length_and_lone_item_form_equal_the_parents_selection(L):
    n = np.array(N_GRID, dtype=np.int64)
    for k in knob_grid("row_max", "row_fe"):
        # batch_fill: n_sets <= e->row_max ? LB_PK_CHUNK_SMALL : LB_PK_CHUNK; lb_fp12_product_is_one: e->row_fe && device_alone(e)
        want = [n <= k.row_max, np.full(len(n), FE_ROW if k.row_fe else FE_WAVE), np.full(len(n), FE_WAVE)]
        same(call(L.c_pipe_misc, k, len(n), [n.astype(np.uint32)], 3), want, ["pk_chunks_small", "fe alone", "fe load"], k, [n])


# ---------------------------------------------------------------------------- 2. the environment table
def env_knobs(L, env):
    out = np.zeros(len(VARS), dtype=np.int64)
    L.c_pipe_env("\n".join("%s=%s" % kv for kv in env.items()).encode(), out.ctypes.data_as(I64P))
    return K(**dict(zip(FIELDS, out.tolist())))


def test_environment_parsing(L):
    out = np.zeros(len(VARS), dtype=np.int64)
    L.c_pipe_knob_defaults(out.ctypes.data_as(I64P))
    assert dict(zip(FIELDS, out.tolist())) == DEFAULTS
    assert vars(env_knobs(L, {})) == DEFAULTS
    strings = ["0", "1", "1000000000", "lane", "g8", "bogus"]
    # what the getenv lines of lb_engine_create_ex gave, by the kind of line
    count = dict(zip(strings, [0, 1, 1000000000, 0, 0, 0]))      # (uint32_t)strtoul(v, nullptr, 10)
    flag = dict(zip(strings, [0, 1, 1, 0, 0, 0]))                # std::atoi(v) != 0
    form = dict(zip(strings, [0, 0, 0, 1, 2, 0]))                # !strcmp(v, "lane") ? 1 : !strcmp(v, "g8") ? 2 : 0
    expected = {"LB_MILLER_WAVE_MAX": count, "LB_ROW_MAX": count, "LB_ROW_FE": flag, "LB_MILLER_LDS3_MAX": count,
                "LB_MILLER_FORM": form, "LB_HASH_G8_MAX": count, "LB_HASH_ROW_MAX": count, "LB_DEC_ROW_MAX": count,
                "LB_SUBGROUP_G8_MAX": count, "LB_SMALL_S_MAX": count, "LB_SMALL_S_G8_MAX": count,
                "LB_SEARCH_SMALL_MAX": count, "LB_SMSM_FORM": form, "LB_MSM_G8": flag,
                "LB_ALONE": flag}                                # std::atoi(v) != 0 ? 1 : 0; unset: -1
    assert set(expected) == set(VARS)
    for var, by_string in expected.items():
        for s, want in by_string.items():
            got = vars(env_knobs(L, {var: s}))
            assert got == {**DEFAULTS, VARS[var][0]: want}, (var, s)
    # variables of the engine that select no form leave the knobs alone
    assert vars(env_knobs(L, {"LB_SEARCH_CHUNK": "1", "LB_HASH_ROW_CAREFUL": "1", "LB_ROOT_SHUFFLE": "0"})) == DEFAULTS


# ---------------------------------------------------------------------------- 3. the GPU tests' recipes
def batch_plan(L, k, n, alone, **shape):
    s = dict(nc=n, n_comb=0, indexed=0, routed=0, scalars=1, unblinded=1, shuffle=1)
    s.update(shape)
    flags = s["indexed"] | s["routed"] << 1 | s["scalars"] << 2 | s["unblinded"] << 3 | s["shuffle"] << 4 | int(alone) << 5
    one = lambda v, t=np.uint32: np.array([v], dtype=t)  # noqa: E731
    got = call(L.c_pipe_batch, k, 1, [one(n), one(s["nc"]), one(s["n_comb"]), one(flags, np.uint8)], 12)
    return dict(zip(BATCH_FIELDS, got[0].tolist()))


def root_plan(L, k, n, nuh, alone, alone_hash, alone_miller, lo=1):
    one = lambda v, t=np.uint32: np.array([v], dtype=t)  # noqa: E731
    flags = int(alone) | int(alone_hash) << 1 | int(alone_miller) << 2
    got = call(L.c_pipe_roots, k, 1, [one(n), one(nuh), one(lo), one(flags, np.uint8)], 4)
    return dict(zip(["hash_map", "hash_fin", "miller", "tree"], got[0].tolist()))


def samples(k):
    """the values device_alone can return on an engine with these knobs: LB_ALONE pins every sample"""
    return [bool(k.alone_force)] if k.alone_force >= 0 else [False, True]


def test_recipes_of_test_miller28_gpu(L):
    """k_miller_lane<3>, k_miller_lane<2> and k_miller_g8 at 1, 64 and 65 distinct roots, one set each"""
    big = str(BIG)
    pin = {"LB_ALONE": "0", "LB_ROW_FE": "0", "LB_MILLER_WAVE_MAX": "0"}
    forms = {"lane3": ({**pin, "LB_MILLER_FORM": "lane", "LB_MILLER_LDS3_MAX": big}, MILLER_LANE3),
             "lane2": ({**pin, "LB_MILLER_FORM": "lane", "LB_MILLER_LDS3_MAX": "0"}, MILLER_LANE2),
             "g8": ({**pin, "LB_MILLER_FORM": "g8", "LB_MILLER_LDS3_MAX": big}, MILLER_G8)}
    for name, (env, want) in forms.items():
        k = env_knobs(L, env)
        for n in (1, 64, 65):
            for a in samples(k):
                assert root_plan(L, k, n, n, a, a, a)["miller"] == want, (name, n)


def test_recipes_of_test_subgroup28_gpu(L):
    """k_sig_subgroup (lone) and k_sig_subgroup_g8 for 130, 64 and 1 sets, whatever device_alone samples"""
    for env, want in (({"LB_SUBGROUP_G8_MAX": "0", "LB_ROW_FE": "0"}, SUBGROUP_LANE),
                      ({"LB_SUBGROUP_G8_MAX": str(BIG), "LB_ROW_FE": "0"}, SUBGROUP_G8)):
        k = env_knobs(L, env)
        for n in (130, 13, 64, 1):
            for a in samples(k):
                for scalars in (0, 1):
                    assert batch_plan(L, k, n, a, scalars=scalars)["subgroup"] == want, (env, n, a)


def test_recipes_of_test_edge_points_gpu(L):
    """k_decompress_sigs under LB_ALONE=0, k_decompress_sigs_row under LB_ALONE=1 LB_ROW_FE=1, for the
    one-set batches and for the interleaved batch of every g2c96 record"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "edge_points.json")))
    n_all = 2 * len([r for r in fx["records"] if r["kind"] == "g2c96"]) + 1
    for env, want in (({"LB_ALONE": "0"}, DEC_LANE), ({"LB_ALONE": "1", "LB_ROW_FE": "1"}, DEC_ROW)):
        k = env_knobs(L, env)
        for n in (1, n_all):
            for a in samples(k):
                assert batch_plan(L, k, n, a, scalars=0)["decode"] == want, (env, n)


def test_recipes_of_test_forgeries_gpu(L):
    """the nine-set batch of edge_run: "lane" runs the one-lane forms and the bucket MSM for S, "alone" the row forms"""
    lane = env_knobs(L, dict(LB_ALONE="0", LB_MILLER_WAVE_MAX="0", LB_HASH_G8_MAX="0", LB_SUBGROUP_G8_MAX="0",
                             LB_SMALL_S_MAX="0", LB_SMALL_S_G8_MAX="0", LB_SEARCH_SMALL_MAX="0"))
    assert samples(lane) == [False]
    n = 9
    for nuh in (8, 9):  # the negated pair shares a root
        b = batch_plan(L, lane, n, False)
        assert (b["decode"], b["subgroup"], b["ssum"], b["fe"], b["gsum"]) == \
            (DEC_LANE, SUBGROUP_LANE, SSUM_BUCKET_MSM, FE_WAVE, GSUM_CHUNKS)
        r = root_plan(L, lane, n, nuh, False, False, False)
        assert (r["hash_map"], r["hash_fin"], r["miller"], r["tree"]) == (HMAP_LANE, HFIN_LANE, MILLER_LANE3, FE_WAVE)
    assert call(L.c_pipe_search_round, lane, 1, [np.array([1], np.uint32), np.array([9], np.uint32),
                                                 np.array([0], np.uint8)], 2)[0, 0] == SRCH_BUCKET_MSM
    alone = env_knobs(L, {"LB_ALONE": "1"})
    assert samples(alone) == [True]
    for nuh in (8, 9):
        b = batch_plan(L, alone, n, True)
        assert (b["decode"], b["subgroup"], b["ssum"], b["fe"], b["gsum"], b["pk_blind"]) == \
            (DEC_ROW, SUBGROUP_W4, SSUM_PAR_W4, FE_ROW, GSUM_WAVE, PKB_SPLIT_ROWP)
        r = root_plan(L, alone, n, nuh, True, True, True, lo=8)
        assert (r["hash_map"], r["hash_fin"], r["miller"], r["tree"]) == (HMAP_ROW, HFIN_ROW, MILLER_ROW, FE_ROW)


def test_recipes_of_test_gpu_parity_row_engine(L):
    """test_row_engine_forms_agree under LB_ALONE=1 over c1 (128 sets), c2 (131) and c3 (19 456 sets, about
    1 150 roots): the row forms by default; none with LB_ROW_FE=0 LB_ROW_MAX=0 LB_HASH_ROW_MAX=0; with
    LB_ROW_MAX=64 LB_HASH_ROW_MAX=2^20 the cofactor clearing by rows at every root count, the Miller loops and
    tree levels by rows up to 64 items, and ML(-G1, S) and the root check / partial by rows in both"""
    shapes = ((128, 128), (131, 131), (131, 4), (19456, 1153))
    base = {"LB_ALONE": "1", "LB_HASH_ROW_CAREFUL": "0"}
    k = env_knobs(L, {**base, "LB_ROW_FE": "1"})
    for n, nuh in shapes:
        r = root_plan(L, k, n, nuh, True, True, True, lo=256)
        assert batch_plan(L, k, n, True)["fe"] == FE_ROW and r["tree"] == FE_ROW
        assert (r["hash_fin"], r["miller"]) == ((HFIN_ROW, MILLER_ROW) if nuh <= 256 else (HFIN_G8, MILLER_WAVE))
    k = env_knobs(L, {**base, "LB_ROW_FE": "0", "LB_ROW_MAX": "0", "LB_HASH_ROW_MAX": "0"})
    for n, nuh in shapes:
        r = root_plan(L, k, n, nuh, True, True, True, lo=1)
        b = batch_plan(L, k, n, True)
        assert (b["fe"], b["decode"], r["tree"], r["hash_map"], r["hash_fin"], r["miller"]) == \
            (FE_WAVE, DEC_LANE, FE_WAVE, HMAP_LANE, HFIN_G8, MILLER_WAVE)
        assert b["subgroup"] != SUBGROUP_W4 and b["ssum"] != SSUM_PAR_W4 and b["pk_blind"] != PKB_SPLIT_ROWP
    k = env_knobs(L, {**base, "LB_ROW_FE": "1", "LB_ROW_MAX": "64", "LB_HASH_ROW_MAX": str(1 << 20), "LB_HASH_ROW_CAREFUL": "1"})
    for n, nuh in shapes:
        r64, r128 = (root_plan(L, k, n, nuh, True, True, True, lo=lo) for lo in (64, 128))
        assert batch_plan(L, k, n, True)["fe"] == FE_ROW
        assert (r64["hash_map"], r64["hash_fin"], r64["tree"], r128["tree"]) == (HMAP_ROW, HFIN_ROW, FE_ROW, FE_WAVE)
        assert r64["miller"] == (MILLER_ROW if nuh <= 64 else MILLER_WAVE)


def test_recipes_of_test_gpu_parity_per_root_forms(L):
    """test_per_root_kernel_forms_agree over c2 (131 sets) and c3 / c3_mixed (19 456 sets, about 1 150 roots):
    under its LB_ALONE=0 the six settings select the forms its comments name.  Without the pin, an engine
    alone on the device ran c2 through the row forms in all six (the last assertion)."""
    big = str(BIG)
    one = lambda v, t=np.uint32: np.array([v], dtype=t)  # noqa: E731
    settings = (  # lim, s_g8, mform, msm_g8, lds3 -> Miller loop, cofactor clearing, subgroup check, S, reduction
        (("0", "0", "lane", "1", big), (MILLER_LANE3, HFIN_LANE, SUBGROUP_LANE, SSUM_BUCKET_MSM, MSMR_WINDOW_HORNER)),
        (("0", "0", "g8", "1", big), (MILLER_G8, HFIN_LANE, SUBGROUP_LANE, SSUM_BUCKET_MSM, MSMR_WINDOW_HORNER)),
        ((big, "0", "g8", "1", big), (MILLER_WAVE, HFIN_G8, SUBGROUP_G8, SSUM_TERMS_LANE, MSMR_WINDOW_HORNER)),
        ((big, big, "lane", "1", big), (MILLER_WAVE, HFIN_G8, SUBGROUP_G8, SSUM_TERMS_G8, MSMR_WINDOW_HORNER)),
        (("0", "0", "lane", "0", big), (MILLER_LANE3, HFIN_LANE, SUBGROUP_LANE, SSUM_BUCKET_MSM, MSMR_REDUCE)),
        (("0", "0", "lane", "1", "0"), (MILLER_LANE2, HFIN_LANE, SUBGROUP_LANE, SSUM_BUCKET_MSM, MSMR_WINDOW_HORNER)))
    for (lim, s_g8, mform, msm_g8, lds3), want in settings:
        env = {"LB_MSM_G8": msm_g8, "LB_MILLER_LDS3_MAX": lds3, "LB_MILLER_FORM": mform, "LB_MILLER_WAVE_MAX": lim,
               "LB_HASH_G8_MAX": lim, "LB_SUBGROUP_G8_MAX": lim, "LB_SMALL_S_MAX": lim, "LB_SMALL_S_G8_MAX": s_g8,
               "LB_SEARCH_SMALL_MAX": lim}
        k = env_knobs(L, {**env, "LB_ALONE": "0"})
        for n, nuh in ((131, 131), (131, 4), (19456, 1153)):
            b = batch_plan(L, k, n, False, indexed=1)
            r = root_plan(L, k, n, nuh, False, False, False)
            msm = call(L.c_pipe_msm, k, 1, [one(8 * n, np.uint64), one(32), one(2048), one(0, np.uint8)], 2)[0]
            assert (r["miller"], r["hash_fin"], b["subgroup"], b["ssum"], msm[1]) == want, (env, n, nuh)
        k = env_knobs(L, env)
        assert samples(k) == [False, True]
        assert root_plan(L, k, 131, 131, True, True, True)["miller"] == MILLER_ROW
        assert batch_plan(L, k, 131, True, indexed=1)["subgroup"] == SUBGROUP_W4
