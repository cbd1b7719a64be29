"""The invalid-set search's planner and interpreter (lodestar_amd/csrc/lb_search_plan.h: what a round
launches and what its results mean) on the CPU: build/lb_search_harness.so runs them in the loop of
lb_engine.hip search_invalid against a model device (tests/harness/search_model.h: a set of failing
sets, exact arithmetic), checking the uploaded tables of every launch set on the way.  The search
must name exactly the failing sets, never reach the round limit, and fail closed when the model lies;
then the helper for blocks of at most 64, the map from failing positions to jobs, and a stand-alone
program of the same cases under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC, R1_PLAIN, RS = 1, 2, 4
LIE_NONE, LIE_PASS, LIE_TOUT, LIE_STALL = 0, 1, 2, 3
F_RS_PATH, F_W4, F_SMALL = 1, 2, 4
U32P = ctypes.POINTER(ctypes.c_uint32)


def load():
    from lodestar_amd.build import build_search_harness
    lib = ctypes.CDLL(build_search_harness(verbose=False))
    u, i = ctypes.c_uint32, ctypes.c_int32
    lib.c_search_const.argtypes = [u]
    lib.c_search_const.restype = u
    lib.c_search_run.argtypes = [u, u, U32P, ctypes.c_char_p, u, u, i, U32P, u, U32P, u, U32P, ctypes.c_char_p, u]
    lib.c_search_run.restype = i
    lib.c_blocks64.argtypes = [U32P, u, U32P, U32P, U32P]
    lib.c_blocks64.restype = u
    lib.c_search_jobs.argtypes = [u, U32P, U32P, u, U32P, u, ctypes.POINTER(i)]
    lib.c_search_jobs.restype = None
    return lib


@pytest.fixture(scope="module")
def L():
    return load()


def _p(a):
    return a.ctypes.data_as(U32P)


def run(lib, roots, bad, flags=0, small_max=32768, lie=LIE_NONE):
    """(sets found in the order found, trace rows [round, nodes, checks, tests, form bits], rounds entered);
    asserts that no table invariant was violated"""
    roots = np.ascontiguousarray(roots, dtype=np.uint32)
    n, nu = len(roots), int(roots.max()) + 1
    assert len(np.unique(roots)) == nu
    flag = np.zeros(n, dtype=np.uint8)
    flag[list(bad)] = 1
    pos = np.zeros(2 * n + 16, dtype=np.uint32)
    trace = np.zeros(5 * 4096, dtype=np.uint32)
    info = np.zeros(3, dtype=np.uint32)
    msg = ctypes.create_string_buffer(4096)
    rc = lib.c_search_run(n, nu, _p(roots), flag.tobytes(), flags, small_max, lie, _p(pos), len(pos), _p(trace),
                          len(trace), _p(info), msg, len(msg))
    assert rc == 0, (rc, msg.value.decode())
    return pos[:info[0]].tolist(), trace[:5 * info[1]].reshape(-1, 5).tolist(), int(info[2])


def exact(lib, roots, bad, **kw):
    found, trace, rounds = run(lib, roots, bad, **kw)
    assert sorted(found) == sorted(bad), (len(roots), sorted(bad), sorted(found), kw)  # no duplicates either
    assert rounds <= lib.c_search_const(3)
    return trace, rounds


def by_first_occurrence(which):
    """roots renumbered by first occurrence, as k_msg_uid numbers them in input order"""
    _, first, inv = np.unique(which, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.uint32)
    rank[np.argsort(first)] = np.arange(len(first), dtype=np.uint32)
    return rank[inv]


def random_layout(rng, n, nu):
    roots = np.concatenate([np.arange(nu), rng.integers(0, nu, size=n - nu)]).astype(np.uint32)
    if rng.integers(0, 3) == 0 and nu > 1:  # skewed: most sets under one root
        big = rng.integers(0, nu)
        roots[nu:][rng.random(n - nu) < 0.8] = big
    rng.shuffle(roots)
    return by_first_occurrence(roots)


def test_constants_are_the_kernels(L):
    src = open(os.path.join(ROOT, "lodestar_amd", "csrc", "lb_kernels.h")).read()
    assert "#define LB_WT_MAX %d " % L.c_search_const(0) in src
    assert [L.c_search_const(k) for k in (1, 2, 3)] == [16384, 1024, 64]


def test_random_layouts_name_exactly_the_failing_sets(L):
    """2 304 layouts: n 1 .. 5 000, nu 1 .. n, every combination of spec_on, r1_plain, rs and the three
    search_small_max values 96 times, 1 to 6 failing sets (sometimes many; the search runs only after a
    failing root check, so there is always one)"""
    rng = np.random.default_rng(0x5EA2C4)
    combos = [(f, sm) for f in range(8) for sm in (0, 64, 32768)]
    forms = set()
    for it in range(96 * len(combos)):
        flags, small_max = combos[it % len(combos)]
        n = int(rng.integers(1, 5001)) if it % 4 else int(rng.integers(1, 200))
        nu = int(rng.integers(1, n + 1)) if it % 3 else int(rng.integers(1, min(n, 8) + 1))
        roots = random_layout(rng, n, nu)
        k = int(rng.integers(1, 7)) if it % 16 else int(rng.integers(1, n + 1))
        bad = set(rng.choice(n, size=min(k, n), replace=False).tolist())
        trace, _ = exact(L, roots, bad, flags=flags, small_max=small_max)
        forms |= {row[4] for row in trace}
    # every form of a round was planned somewhere: root-level, bucket MSM with 4 and with 6 windows, small
    assert {F_RS_PATH | F_SMALL, F_RS_PATH | F_W4 | F_SMALL, F_W4, 0, F_SMALL, F_W4 | F_SMALL} <= forms, forms


@pytest.mark.parametrize("flags", [0, SPEC, RS, SPEC | R1_PLAIN | RS])
def test_root_above_the_weighted_part_cap(L, flags):
    """2 200 sets over 2 roots, three failing (tests/test_gpu_parity.py test_search_root_above_weighted_part_cap):
    a weighted test over parts of two sets, then over the named part's sets"""
    rng = np.random.default_rng(37)
    roots = by_first_occurrence(rng.integers(0, 2, size=2200))
    assert max(np.bincount(roots)) > L.c_search_const(0)
    for small_max in (0, 64, 32768):
        exact(L, roots, {3, 1099, 2150}, flags=flags, small_max=small_max)


@pytest.mark.parametrize("nu", [1, 2, 64, 65, 4096, 4097])
def test_root_counts_at_the_tree_and_subtree_edges(L, nu):
    rng = np.random.default_rng(nu)
    for n in (nu, nu + 1, min(5000, 2 * nu + 37)):
        roots = random_layout(rng, n, nu)
        for flags in range(8):
            for bad in ({0}, {n - 1}, {0, n - 1}, set(rng.choice(n, size=min(n, 3), replace=False).tolist())):
                exact(L, roots, bad, flags=flags, small_max=(0, 64, 32768)[flags % 3])


def test_two_failing_roots_in_one_64_root_subtree(L):
    """200 sets over 130 roots, two failing sets under roots 3 and 40 (one subtree of 64 roots) and one
    under root 100: the subtree's weighted test matches nothing and its roots are checked one by one in
    ONE round, so the search ends as fast as with one failing root per subtree"""
    rng = np.random.default_rng(5)
    roots = random_layout(rng, 200, 130)
    pick = [int(np.nonzero(roots == u)[0][0]) for u in (3, 40, 100)]
    for flags in range(8):
        trace, rounds = exact(L, roots, set(pick), flags=flags, small_max=64)
        assert rounds <= 5, trace
        # the round after the subtree's failed test: 64 direct checks of its roots
        assert any(row[2] == 64 for row in trace), trace


def test_every_set_failing(L):
    rng = np.random.default_rng(300)
    for nu in (1, 7, 300):
        for flags in range(8):
            exact(L, random_layout(rng, 300, nu), set(range(300)), flags=flags, small_max=(0, 64, 32768)[flags % 3])


def test_first_and_last_position(L):
    rng = np.random.default_rng(11)
    for n, nu in ((1, 1), (2, 1), (2, 2), (1025, 1), (1027, 3), (5000, 70), (5000, 5000)):
        roots = random_layout(rng, n, nu)
        order = np.argsort(roots, kind="stable")  # members: sets sorted by root, input order inside a root
        for bad in ({int(order[0])}, {int(order[-1])}, {int(order[0]), int(order[-1])}):
            for flags in (0, SPEC, SPEC | RS, R1_PLAIN):
                exact(L, roots, bad, flags=flags)


def test_instance_budget_splits_a_round(L):
    """5 000 sets over 2 500 roots, every set failing: the second round's failing subtrees carry more
    than kMaxMsm MSM instances, so the round runs as several launch sets (each past the budget only
    by its last whole node: checked on every launch set)"""
    roots = by_first_occurrence(np.repeat(np.arange(2500), 2))
    for flags in (0, SPEC, RS):
        trace, _ = exact(L, roots, set(range(5000)), flags=flags)
        per_round = np.bincount([row[0] for row in trace])
        assert per_round.max() > 1, trace


def test_blocks_of_at_most_64(L):
    rng = np.random.default_rng(64)
    for lens in ([0], [1], [64], [65], [128, 0, 1, 63, 64, 65, 200], rng.integers(0, 300, size=50).tolist()):
        pre = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.uint32)  # a prefix array need not start at 0
        cnt = len(lens)
        cap = int(pre[-1] - pre[0]) + cnt + 1
        blo, bhi, bo = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        bo = np.zeros(cnt + 1, dtype=np.uint32)
        nbk = L.c_blocks64(_p(pre), cnt, _p(blo), _p(bhi), _p(bo))
        assert bo[0] == 0 and bo[cnt] == nbk
        for j in range(cnt):
            blocks = [(int(blo[b]), int(bhi[b])) for b in range(bo[j], bo[j + 1])]
            assert all(0 < h - l <= 64 for l, h in blocks)
            assert len(blocks) == (lens[j] + 63) // 64
            # they tile [pre[j], pre[j + 1]) in order
            edges = [pre[j]] + [h for _, h in blocks]
            assert [l for l, _ in blocks] == edges[:-1] and edges[-1] == pre[j + 1]


def test_lying_model_every_direct_check_passes(L):
    """fail closed: a multi node none of whose children fails is condemned whole (here the root)"""
    rng = np.random.default_rng(1)
    roots = random_layout(rng, 500, 40)
    found, trace, rounds = run(L, roots, {17}, lie=LIE_PASS)
    assert sorted(found) == list(range(500)) and rounds == 1 and len(trace) == 1


def test_lying_model_tests_return_out_of_range_children(L):
    """an out-of-range tout (above f, or negative) sends the node to direct checks: the search still ends
    with exactly the failing sets, by direct checks alone"""
    rng = np.random.default_rng(2)
    for n, nu in ((500, 40), (2200, 2), (3000, 3000)):
        roots = random_layout(rng, n, nu)
        bad = set(rng.choice(n, size=4, replace=False).tolist())
        honest, _ = exact(L, roots, bad, flags=SPEC)
        lied, _ = exact(L, roots, bad, flags=SPEC, lie=LIE_TOUT)
        assert sum(row[2] for row in lied) > sum(row[2] for row in honest)


def test_lying_model_nodes_never_shrink(L):
    """the round's results are dropped and the same node fails again: after kMaxRounds rounds the limit
    condemns what is left, whole"""
    rng = np.random.default_rng(3)
    roots = random_layout(rng, 500, 40)
    found, trace, rounds = run(L, roots, {17, 300}, lie=LIE_STALL)
    assert rounds == L.c_search_const(3) + 1 and len(trace) == L.c_search_const(3)
    assert sorted(found) == list(range(500))


def test_failing_positions_to_jobs(L):
    """over multi-set jobs (some empty): a job becomes 0 iff it was 1 and holds a failing set"""
    rng = np.random.default_rng(4)
    for _ in range(50):
        nj = int(rng.integers(1, 40))
        sizes = rng.integers(0, 5, size=nj)
        job_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        n = int(job_off[-1])
        if n == 0:
            continue
        members = rng.permutation(n).astype(np.uint32)
        before = rng.choice([1, 1, 1, -3, -6, 0], size=nj).astype(np.int32)
        bad_pos = rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).astype(np.uint32)
        bad_sets = set(members[bad_pos].tolist())
        out = before.copy()
        L.c_search_jobs(n, _p(members), _p(bad_pos), len(bad_pos), _p(job_off), nj, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        for j in range(nj):
            holds = any(i in bad_sets for i in range(job_off[j], job_off[j + 1]))
            assert out[j] == (0 if holds and before[j] == 1 else before[j])


def test_search_plan_under_sanitizers(tmp_path):
    """tests/native/search_plan_check.cpp: a few hundred of the same cases in a program of its own, built
    with -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "search_plan_check"
    subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "tests", "harness"),
                    os.path.join(ROOT, "tests", "native", "search_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search_plan_check: failures 0" in out.stdout
