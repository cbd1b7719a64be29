"""r PK from the resident table's fixed-base comb (k_comb_fill at registration, k_pk_blind_comb per
batch, the ladder over the compacted rest) against the GLV ladder over every set (LB_PK_COMB=0):
the same per-job codes, equal to the workload's expected codes, and -- with the blinding words
pinned -- the same Fp12 partial byte for byte.  Every case runs under LB_ALONE=0: the row forms a
small batch takes on an idle device keep the ladder, so the comb would not run at these sizes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAD48 = bytes([0x9F]) + b"\xff" * 47   # x >= p: BLST_BAD_ENCODING
INF48 = bytes([0xC0]) + bytes(47)      # the point at infinity
N_POOL = 16


def att(v):
    from lodestar_amd.workloads import SetSpec
    return [SetSpec([v], 3)]


def agg_job(v, members):
    """an aggregate-and-proof call: selection proof, aggregator signature, the aggregate"""
    from lodestar_amd.workloads import SetSpec
    return [SetSpec([v], 5), SetSpec([v], 6), SetSpec(list(members), 3)]


def run_on_off(monkeypatch, jobs, register, override=None, env=(), coverage=None, unpinned_too=False):
    """`register(engine, pool)` fills the table; the specs' validator ids are table indices (row t
    holds pool key t mod N_POOL unless `register` says otherwise).  Returns nothing: asserts."""
    from lodestar_amd.engine import Engine, PackedJobs
    from lodestar_amd import workloads as W
    monkeypatch.setenv("LB_ALONE", "0")
    for k, v in env:
        monkeypatch.setenv(k, v)
    wl = sc = ip = None
    outs = []
    for comb in ("1", "0"):
        monkeypatch.setenv("LB_PK_COMB", comb)
        with Engine(0) as e:
            if wl is None:  # signed once, on the first engine
                pool = W.KeyPool(e, N_POOL)
                wl = W.build(e, jobs, "pk_comb", keys=pool)
                p = wl.packed
                flat = np.fromiter((v for j in jobs for s in j for v in s.validators), dtype=np.int64)
                ip = PackedJobs(job_off=p.job_off, pk_off=p.pk_off, pubkeys=None, msgs=p.msgs, sigs=p.sigs,
                                sig_sizes=p.sig_sizes, pk_indices=flat.astype(np.uint32))
                sc = np.random.default_rng(7).integers(1, 1 << 63, size=p.n_sets, dtype=np.uint64)
            register(e, pool)
            n_table = e.pubkey_table_size()
            want_cov = 0 if comb == "0" else (n_table if coverage is None else coverage)
            assert e.pubkey_comb_size() == want_cov
            # the sets the routing hands to k_pk_blind_comb: one key, its index inside the coverage
            n_comb = sum(1 for j in jobs for s in j if len(s.validators) == 1 and s.validators[0] < want_cov)
            assert n_comb > 0 or comb == "0"
            b = e.upload(ip)
            try:
                got = np.asarray(b.verify(scalars=sc))
                part = bytes(b.partial(scalars=sc)[0])
                free = np.asarray(b.verify()) if unpinned_too else None
            finally:
                b.free()
            # ... and the comb kernel did run over them in each of the pipeline runs above (a silent
            # fall-back to the ladder would make the on/off comparison compare nothing)
            assert e.pubkey_comb_sets() == n_comb * (3 if unpinned_too else 2)
        exp = wl.expected.copy()
        for j, code in (override or {}).items():
            exp[j] = code
        assert np.array_equal(got, exp), (comb, got, exp)
        if free is not None:
            assert np.array_equal(free, exp), (comb, free, exp)
        outs.append((got, part))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def register_pool(rows):
    def reg(e, pool):
        first, st = e.pubkey_table_append(np.ascontiguousarray(pool.pk96[np.arange(rows) % N_POOL]))
        assert first == 0 and not any(st)
    return reg


def test_one_single_key_set(monkeypatch):
    """(a) one set; also unpinned, where the engine verifies it unblinded (the word 1: r PK = PK)"""
    run_on_off(monkeypatch, [att(3)], register_pool(N_POOL), unpinned_too=True)


def test_65_single_key_sets(monkeypatch):
    """(b) a second wave with one live lane"""
    run_on_off(monkeypatch, [att(i % N_POOL) for i in range(65)], register_pool(N_POOL))


@pytest.mark.parametrize("row_max", [None, "0"])
def test_mixed_batch_with_rejected_keys(monkeypatch, row_max):
    """(c) two 3-set jobs whose third sets aggregate 2 and 17 keys (chunks of 16 keys with
    LB_ROW_MAX=0: two chunks; of 4 at the default) and a lone attestation: 7 sets, 5 for the comb
    and 2 for the ladder.  Then one set over an index >= table_n, one over a key registered as a bad
    encoding, one over a key registered as infinity: each rejects its own job."""
    def reg(e, pool):
        register_pool(N_POOL)(e, pool)
        first, st = e.pubkey_table_append([BAD48, INF48])
        assert first == N_POOL and st == [1, 0]
    jobs = [agg_job(1, [2, 9]), agg_job(4, [(3 * i + 1) % N_POOL for i in range(17)]), att(6),
            att(10 ** 6), att(N_POOL), att(N_POOL + 1)]
    env = () if row_max is None else (("LB_ROW_MAX", row_max),)
    run_on_off(monkeypatch, jobs, reg, override={3: -100, 4: -1, 5: -6}, env=env)


def test_budget_covers_first_8_of_16_keys(monkeypatch):
    """(d) LB_PK_COMB_MB for 8 keys' entries (8 x 72 x 96 B = 0.0527 MiB): keys 0..7 take the comb,
    keys 8..15 the ladder; sets on both sides of the boundary and an aggregate across it."""
    jobs = [att(7), att(8), att(0), att(15), agg_job(7, [7, 8]), agg_job(8, [8, 7])]
    run_on_off(monkeypatch, jobs, register_pool(N_POOL), env=(("LB_PK_COMB_MB", "0.0528"),), coverage=8)


def test_table_growth_carries_the_entries(monkeypatch):
    """(e) 1 000 keys, then 100 more: the table crosses its 1 024-record growth step, the copy
    carries the entries of the first 1 000 and the new keys get theirs."""
    def reg(e, pool):
        first, st = e.pubkey_table_append(np.ascontiguousarray(pool.pk96[np.arange(1000) % N_POOL]))
        assert first == 0 and not any(st)
        first, st = e.pubkey_table_append(np.ascontiguousarray(pool.pk96[np.arange(1000, 1100) % N_POOL]))
        assert first == 1000 and not any(st)
    run_on_off(monkeypatch, [att(5), att(1050), att(999), att(1000), att(1023), att(1024), att(1099)], reg)
