"""BlsGpuVerifier({devices}) of the Node.js host side (lodestar_amd/js/index.js): the dispatch over
several device slots against a mock addon (no GPU), its cost split against distributed.py's, and
the two-slot cases on one GPU - tests/js/test_multidevice.js run with the system node."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_multidevice.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")


def _run(*args):
    if NODE is None:
        pytest.skip("node not installed")
    if not os.path.exists(ADDON):
        from lodestar_amd.build import build_napi
        build_napi(verbose=False)
    r = subprocess.run([NODE, SCRIPT, *args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_js_multidevice_dispatch_cpu():
    """engine creation on 8 devices, the balanced split, the threshold, busy slots, isolation, close(),
    the device-less constructor and devices: "all", against a mock addon (modules.addon)"""
    assert "js multidevice cpu ok" in _run("cpu")


def _random_job_lists():
    """50 seeded job lists: per job the key count of each of its sets (1-set gossip jobs, 3-set
    aggregate jobs with a 256-key set, block chunks, empty jobs, odd aggregates)"""
    rng = np.random.default_rng(20240607)
    lists = []
    for n in range(50):
        jobs = []
        for _ in range(int(rng.integers(0 if n == 0 else 1, 90))):
            kind = int(rng.integers(0, 10))
            if kind < 5:
                jobs.append([1])
            elif kind < 8:
                jobs.append([1, 1, 256])
            elif kind == 8:
                jobs.append([int(k) for k in rng.integers(1, 600, int(rng.integers(1, 140)))])
            else:
                jobs.append([] if rng.random() < 0.3 else [1] * int(rng.integers(1, 129)))
        lists.append(jobs)
    return lists


def test_js_and_python_split_agree(tmp_path):
    """splitByCost(jobs, k) cuts where distributed.shard_jobs_by_cost does, for k = 1..8"""
    from lodestar_amd.distributed import shard_jobs_by_cost
    lists = _random_job_lists()
    p = tmp_path / "lists.json"
    p.write_text(json.dumps(lists))
    out = _run("split", str(p)).strip().splitlines()
    assert out[-1] == "js multidevice split ok"
    got = json.loads(out[-2])
    assert len(got) == 50
    differing = 0
    for jobs, per_k in zip(lists, got):
        job_off = np.concatenate([[0], np.cumsum([len(j) for j in jobs])]).astype(np.int64)
        pk_off = np.concatenate([[0], np.cumsum([k for j in jobs for k in j])]).astype(np.int64)
        for k in range(1, 9):
            want = [list(shard_jobs_by_cost(job_off, pk_off, k, r)) for r in range(k)]
            assert per_k[k - 1] == want, (jobs, k)
            assert want[0][0] == 0 and want[-1][1] == len(jobs)
            assert all(a[1] == b[0] for a, b in zip(want, want[1:]))
            differing += len(set(map(tuple, want))) > 1
    assert differing > 300  # the lists do get cut


def _signed_file(engine, tmp_path):
    """8 keys, 16 roots and every key's signature of every root (lb_sign), for the JS side"""
    from lodestar_amd.workloads import interop_sk
    sks = [interop_sk(i) for i in range(8)]
    _, pk96 = engine.sk_to_pk(sks)
    roots = np.frombuffer(b"".join(bytes([r + 1]) * 32 for r in range(16)), np.uint8).reshape(16, 32)
    sigs = engine.sign([sk for sk in sks for _ in range(16)], np.tile(roots, (8, 1)))
    p = tmp_path / "signed.json"
    p.write_text(json.dumps({"keys": [bytes(k).hex() for k in pk96], "roots": [bytes(r).hex() for r in roots],
                             "sigs": [[bytes(sigs[16 * k + r]).hex() for r in range(16)] for k in range(8)]}))
    return str(p)


@pytest.mark.gpu
def test_js_golden_cases_on_two_slots_gpu():
    assert "js multidevice gpu golden ok" in _run("gpu", "golden")


@pytest.mark.gpu
def test_js_split_package_gpu(engine, tmp_path):
    """512 one-set jobs cut over two slots of one GPU: both slots used, 510 true, one false, one
    BLST_INVALID_SIZE, the same verdicts as a verifier without `devices`"""
    assert "js multidevice gpu split ok" in _run("gpu", "split", _signed_file(engine, tmp_path))


@pytest.mark.gpu
def test_js_registered_keys_on_every_slot_gpu(engine, tmp_path):
    assert "js multidevice gpu keys ok" in _run("gpu", "keys", _signed_file(engine, tmp_path))


@pytest.mark.gpu
def test_js_devices_all_gpu():
    assert "js multidevice gpu all ok" in _run("gpu", "all")


@pytest.mark.gpu
def test_js_close_leaves_no_engine_gpu():
    assert "js multidevice gpu close ok" in _run("gpu", "close")
