"""The JS twin of tests/test_ssz_sets_gpu.py: getBlockSignatureSetsFromSsz (lodestar_amd/js/signing_roots.js,
addon.blockSetsFromSsz) on blocks encoded by tests/ssz_codec.py, against the JS JSON walk: the K3 block, the
every-operation block, one block per fork, a malformed block between them and both branches of the sync rule,
all in one call (tests/js/test_ssz_sets.js)."""
import copy
import json
import os
import shutil
import subprocess

import pytest

import ssz_codec as C
from conftest import ROOT, load_json

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_ssz_sets.js")


@pytest.mark.gpu
def test_js_sets_from_ssz_match_the_json_walk(tmp_path):
    if NODE is None:
        pytest.skip("node not installed")
    k3 = load_json("k3_devnet.json")
    cases = []

    def add(name, blk, fork, error=None, cut=None):
        raw = C.encode_signed_block(blk, fork)
        cases.append({"name": name, "fork": fork, "ssz": (raw if cut is None else raw[:cut]).hex(),
                      "block": C.canonical(blk), "error": error})
    add("k3", k3["signed_block"], 3)
    add("every_operation", C.every_operation_block(k3), 3)
    add("malformed", C.every_operation_block(k3), 3, error="not a well-formed", cut=5000)
    for f in range(3):
        add("fork%d" % f, C.fork_block({"signed_block": C.every_operation_block(k3)}, f), f)
    for name, sig, err in (("sync_empty_infinity", "0xc0" + "00" * 95, None),
                           ("sync_empty_not_infinity", "0xc0" + "00" * 94 + "01",
                            "Empty sync committee signature is not infinity")):
        blk = copy.deepcopy(k3["signed_block"])
        blk["message"]["body"]["sync_aggregate"] = {"sync_committee_bits": "0x" + "00" * 64, "sync_committee_signature": sig}
        add(name, blk, 3, error=err)
    p = tmp_path / "cases.json"
    p.write_text(json.dumps({"k3": {k: k3[k] for k in ("genesis_validators_root", "fork")}, "cases": cases}))
    r = subprocess.run([NODE, SCRIPT, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "js ssz sets ok"
