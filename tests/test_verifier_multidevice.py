"""BlsGpuVerifier(devices=...) of the Python mirror (lodestar_amd/verifier.py): the dispatch over
several device slots against a fake Engine (no GPU), and two slots on one GPU."""
import asyncio
import threading

import pytest

from lodestar_amd import _native as N
from lodestar_amd import verifier as V
from lodestar_amd.distributed import KEY_COST, SET_COST
from lodestar_amd.engine import BlsError, Engine

from conftest import load_json


class FakeEngines:
    """An Engine factory (BlsGpuVerifier(engine_factory=...)) that records what is created.  Its
    engines' verify_jobs block until the test releases them; the per-job code comes from the first
    byte of the job's first signature (1 valid, 0 invalid, anything else -10)."""

    def __init__(self, device_count=8, hold=True):
        self.created = []
        self.n_devices = device_count
        self.lock = threading.Lock()
        self.packages = []          # (engine, [first signing root of each job]) in start order
        self.started = threading.Semaphore(0)
        self.release = threading.Event()
        if not hold:
            self.release.set()

    def device_count(self):
        return self.n_devices

    def __call__(self, device, flags=0):
        e = FakeEngine(self, device, flags, len(self.created))
        self.created.append(e)
        return e

    def wait_started(self, n):
        for _ in range(n):
            assert self.started.acquire(timeout=10), "a package did not start"


class FakeEngine:
    def __init__(self, owner, device, flags, id_):
        self.owner, self.device, self.flags, self.id = owner, device, flags, id_
        self.table = 0
        self.closed = 0
        self.appends = 0

    def _verify(self, jobs):
        with self.owner.lock:
            self.owner.packages.append((self, [j[0].signing_root for j in jobs]))
        self.owner.started.release()
        assert self.owner.release.wait(timeout=10)
        return [{1: 1, 0: 0}.get(j[0].signature[0], -10) for j in jobs]

    def verify_jobs(self, jobs, scalars=None):
        return self._verify(jobs)

    def verify_jobs_indexed(self, jobs, indices, scalars=None):
        return self._verify(jobs)

    def pubkey_table_append(self, keys, validate=False):
        first, self.table = self.table, self.table + len(keys)
        self.appends += 1
        return first, [0] * len(keys)

    def g1_decompress(self, pks48, validate=False):
        return [bytes(96) for _ in pks48], [0] * len(pks48)

    def close(self):
        self.closed += 1


_serial = [0]


def mk_job(n_sets, keys_of_last=0, marker=1):
    """the sets of one job; its serial number is in its signing roots"""
    _serial[0] += 1
    root = _serial[0].to_bytes(32, "little")
    pk = V.PublicKey(b"\x02" * 96)
    sig = bytes([marker]) + bytes(95)
    sets = [V.SingleSignatureSet(pubkey=pk, signing_root=root, signature=sig) for _ in range(n_sets)]
    if keys_of_last:
        sets[-1] = V.AggregatedSignatureSet(pubkeys=[pk] * keys_of_last, signing_root=root, signature=sig)
    return sets


def cost(sets):
    return sum(SET_COST + KEY_COST * (len(s.pubkeys) if s.type == V.SignatureSetType.aggregate else 1) for s in sets)


def mixed_queue():
    """64 jobs: 1-set jobs, 3-set jobs with a 256-key aggregate and one 128-set job, in the order of
    tests/js/test_multidevice.js's mixed queue (the 128-set job is heavier than an eighth of the
    queue; it sits where the eighths around it still hold another job's midpoint, so the 8-way cut
    has no empty range)"""
    order = MIXED_ORDER()
    return [mk_job(128) if c == "B" else mk_job(1) if c == "1" else mk_job(3, 256) for c in order]


def MIXED_ORDER():
    from lodestar_amd.distributed import shard_jobs_by_cost
    for n_one in range(3, 13):
        for pos in range(64):
            order = ["B" if i == pos else "A" for i in range(64)]
            for q in range(n_one):
                at = int((q + 0.5) * 64 // n_one)
                if order[at] == "A":
                    order[at] = "1"
            sets = {"B": [1] * 128, "1": [1], "A": [1, 1, 256]}
            job_off, pk_off = [0], [0]
            for c in order:
                for k in sets[c]:
                    pk_off.append(pk_off[-1] + k)
                job_off.append(job_off[-1] + len(sets[c]))
            if all(hi > lo for lo, hi in (shard_jobs_by_cost(job_off, pk_off, 8, r) for r in range(8))):
                return order
    raise AssertionError("no order of the mixed queue fills all eight ranges")


def run(coro):
    return asyncio.run(coro)


async def submit_all(pool, jobs, opts=None):
    """every job queued in one go, before any runner can take the queue"""
    with pool._lock:
        futs = [asyncio.ensure_future(pool.verify_signature_sets(j, opts)) for j in jobs]
        await asyncio.sleep(0)
    return futs


def assert_cover(packages, jobs):
    roots = [j[0].signing_root for j in jobs]
    ranges = []
    for _, got in packages:
        lo = roots.index(got[0])
        assert got == roots[lo:lo + len(got)], "a package is a contiguous range of the queue"
        ranges.append((lo, lo + len(got)))
    at = 0
    for lo, hi in sorted(ranges):
        assert lo == at, "ranges cover the queue without gap or overlap"
        at = hi
    assert at == len(jobs)
    return ranges


def test_engine_creation_eight_devices():
    async def main():
        f = FakeEngines()
        pool = V.BlsGpuVerifier(devices=range(8), n_engines=1, min_package_sets=16, engine_factory=f)
        assert [(e.device, e.flags) for e in f.created] == [(0, Engine.LATENCY)] + [(d, 0) for d in range(8)]
        assert pool.engine is f.created[0] and pool.engines == f.created[1:]
        pks = pool.register_pubkeys([bytes(96)] * 3)
        assert [e.appends for e in f.created] == [1] * 9
        assert [p.index for p in pks] == [0, 1, 2]
        assert [p.index for p in pool.register_pubkeys([bytes(48)])] == [3]
        f.created[6].table = 99
        with pytest.raises(RuntimeError, match="out of step"):
            pool.register_pubkeys([bytes(96)])
        await pool.close()
        await pool.close()
        assert [e.closed for e in f.created] == [1] * 9
    run(main())


def test_failing_engine_creation_closes_what_was_created():
    f = FakeEngines()

    def make(device, flags=0):
        if device == 5:
            raise BlsError(N.LB_ERR_DEVICE)
        return f(device, flags)
    with pytest.raises(BlsError, match="LB_ERR_DEVICE"):
        V.BlsGpuVerifier(devices=range(8), n_engines=1, min_package_sets=16, engine_factory=make)
    assert [e.closed for e in f.created] == [1] * 6


def test_balanced_split_over_eight_slots():
    async def main():
        f = FakeEngines()
        pool = V.BlsGpuVerifier(devices=range(8), n_engines=1, min_package_sets=16, engine_factory=f)
        jobs = mixed_queue()
        futs = await submit_all(pool, jobs)
        f.wait_started(8)
        assert sorted(e.device for e, _ in f.packages) == list(range(8))
        assert_cover(f.packages, jobs)
        by_root = {j[0].signing_root: cost(j) for j in jobs}
        costs = [sum(by_root[r] for r in got) for _, got in f.packages]
        largest = max(by_root.values())
        assert largest == 128 * (SET_COST + KEY_COST)
        print("package costs", costs)
        assert max(costs) - min(costs) <= largest
        assert pool.stats.packages_per_slot == [1] * 8 and pool.stats.splits == 1
        f.release.set()
        assert await asyncio.gather(*futs) == [True] * 64
        await pool.close()
    run(main())


def test_no_split_below_the_threshold():
    async def main():
        f = FakeEngines()
        jobs = mixed_queue()
        n_sets = sum(len(j) for j in jobs)
        pool = V.BlsGpuVerifier(devices=range(8), n_engines=1, min_package_sets=n_sets + 1, engine_factory=f)
        futs = await submit_all(pool, jobs)
        f.wait_started(1)
        assert len(f.packages) == 1 and len(f.packages[0][1]) == 64
        assert f.packages[0][0].device == 0  # nothing in flight anywhere: the lowest slot
        assert pool.stats.splits == 0
        f.release.set()
        assert await asyncio.gather(*futs) == [True] * 64
        assert pool.stats.batches == 1
        await pool.close()
    run(main())


def test_per_job_codes_and_busy_slots():
    async def main():
        f = FakeEngines(device_count=3)
        pool = V.BlsGpuVerifier(devices="all", n_engines=1, min_package_sets=1, engine_factory=f)
        assert pool.devices == [0, 1, 2]
        first = [mk_job(1, marker=m) for m in (1, 0, 2)] + [mk_job(1) for _ in range(6)]
        futs = await submit_all(pool, first)
        f.wait_started(3)
        assert_cover(f.packages, first)
        # every slot is busy: a second queue waits for a runner
        more = await submit_all(pool, [mk_job(1) for _ in range(3)])
        await asyncio.sleep(0.05)
        assert len(f.packages) == 3
        f.release.set()
        res = await asyncio.gather(*futs, return_exceptions=True)
        assert res[0] is True and res[1] is False and str(res[2]) == "BLST_INVALID_SIZE" and res[3:] == [True] * 6
        assert await asyncio.gather(*more) == [True] * 3
        await pool.close()
    run(main())


def test_close_aborts_queued_awaits_running_and_closes_engines_once():
    async def main():
        f = FakeEngines(device_count=2)
        pool = V.BlsGpuVerifier(devices=[0, 1], n_engines=1, min_package_sets=1000, engine_factory=f)
        flying = await submit_all(pool, [mk_job(1), mk_job(1)])
        f.wait_started(1)
        batch = V.VerifySignatureOpts(batchable=True)
        buffered = await submit_all(pool, [mk_job(1)], batch)
        closing = asyncio.ensure_future(pool.close())
        await asyncio.sleep(0.05)
        assert not closing.done(), "close() waits for the package in flight"
        assert [e.closed for e in f.created] == [0, 0, 0]
        with pytest.raises(V.QueueError, match="^QUEUE_ERROR_QUEUE_ABORTED$"):
            await buffered[0]
        f.release.set()
        await closing
        assert await asyncio.gather(*flying) == [True, True]
        assert [e.closed for e in f.created] == [1, 1, 1]
        await pool.close()
        assert [e.closed for e in f.created] == [1, 1, 1]
        assert len(f.packages) == 1
    run(main())


def test_close_aborts_jobs_queued_behind_a_busy_slot():
    async def main():
        f = FakeEngines(device_count=1)
        pool = V.BlsGpuVerifier(devices=[0], n_engines=1, min_package_sets=16, engine_factory=f)
        flying = await submit_all(pool, [mk_job(1)])
        f.wait_started(1)
        queued = await submit_all(pool, [mk_job(1)])
        closing = asyncio.ensure_future(pool.close())
        with pytest.raises(V.QueueError, match="^QUEUE_ERROR_QUEUE_ABORTED$"):
            await queued[0]
        f.release.set()
        await closing
        assert await flying[0] is True
    run(main())


def test_without_devices_one_slot_takes_the_whole_queue():
    async def main():
        f = FakeEngines(hold=False)
        pool = V.BlsGpuVerifier(device=5, engine_factory=f)
        # today's engines: the pool's two, then the synchronous callers' own, no flags
        assert [(e.device, e.flags) for e in f.created] == [(5, 0)] * 3
        assert pool.engine is f.created[2] and pool.min_package_sets == V.DEFAULT_MIN_PACKAGE_SETS
        jobs = mixed_queue()
        futs = await submit_all(pool, jobs)
        assert await asyncio.gather(*futs) == [True] * 64
        assert len(f.packages) == 1 and pool.stats.packages_per_slot == [1] and pool.stats.splits == 0
        await pool.close()
    run(main())


def test_devices_all_without_a_device():
    with pytest.raises(BlsError, match="^LB_ERR_NO_DEVICE$"):
        V.BlsGpuVerifier(devices="all", engine_factory=FakeEngines(device_count=0))
    with pytest.raises(ValueError):
        V.BlsGpuVerifier(devices=[], engine_factory=FakeEngines())


def test_device_count():
    """lb_device_count through Engine.device_count(): 0 where there is no GPU, never an error"""
    import torch
    n = Engine.device_count()
    if torch.cuda.is_available():
        assert 1 <= n <= torch.cuda.device_count()
    else:
        assert n == 0
        with pytest.raises(BlsError, match="^LB_ERR_NO_DEVICE$"):
            V.BlsGpuVerifier(devices="all")
    assert N.load().lb_abi_version() >= 1


def test_default_min_package_sets_matches_js():
    import os
    import re
    from conftest import ROOT
    js = open(os.path.join(ROOT, "lodestar_amd", "js", "index.js")).read()
    assert int(re.search(r"const DEFAULT_MIN_PACKAGE_SETS = (\d+);", js).group(1)) == V.DEFAULT_MIN_PACKAGE_SETS
    assert V.DEFAULT_MIN_PACKAGE_SETS >= 256 and V.DEFAULT_MIN_PACKAGE_SETS & (V.DEFAULT_MIN_PACKAGE_SETS - 1) == 0


def _sets_from_case(c):
    def pk(h):
        return V.PublicKey(bytes.fromhex(h))
    out = []
    for s in c["sets"]:
        if len(s["pubkeys"]) == 1 and "aggregate" not in c["name"]:
            out.append(V.SingleSignatureSet(pk(s["pubkeys"][0]), bytes.fromhex(s["signing_root"]),
                                            bytes.fromhex(s["signature"])))
        else:
            out.append(V.AggregatedSignatureSet([pk(p) for p in s["pubkeys"]], bytes.fromhex(s["signing_root"]),
                                                bytes.fromhex(s["signature"])))
    return out


@pytest.mark.gpu
def test_golden_cases_on_two_slots_gpu():
    """every golden case through BlsGpuVerifier(devices=[0, 0]), all submitted at once, batchable and not"""
    cases = load_json("jobs.json")["cases"]

    async def outcome(coro):
        try:
            return await coro
        except BlsError as e:
            return e.name

    async def main():
        pool = V.BlsGpuVerifier(devices=[0, 0], n_engines=1, min_package_sets=64)
        try:
            for batchable in (False, True):
                opts = V.VerifySignatureOpts(batchable=batchable)
                got = await asyncio.gather(*[outcome(pool.verify_signature_sets(_sets_from_case(c), opts)) for c in cases])
                for c, g in zip(cases, got):
                    assert g == c["expected"], (c["name"], batchable)
            assert len(pool.stats.packages_per_slot) == 2
        finally:
            await pool.close()
    run(main())
