"""tests/js/test_kzg_recover.js: recoverCellsAndKzgProofs(Many) of lodestar_amd/js/kzg.js.  Without a
GPU: the names and argument validation.  On the GPU: recovery of the degree-70 blob from cells
64 .. 127 gives the bytes of a fixture written by tests/test_kzg_recover.py's helper (cells by the Python
transform, proofs by FK20 on the blob), and a changed 65-cell input throws BLST_VERIFY_FAIL."""
import json
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lodestar_amd import kzg as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_kzg_recover.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")


def _run(*args):
    if NODE is None:
        pytest.skip("node not installed")
    if not os.path.exists(ADDON):
        from lodestar_amd.build import build_napi
        build_napi(verbose=False)
    r = subprocess.run([NODE, SCRIPT, *args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"js kzg recover {args[0]} ok", r.stdout
    return json.loads(lines[-2])


def test_js_names_and_argument_validation():
    assert _run("cpu") == {}


@pytest.mark.gpu
def test_js_recovers_the_fixture_bytes(engine, tmp_path):
    import test_kzg_recover as T
    host = K.Kzg(engine)
    path = tmp_path / "recover.json"
    T.write_js_fixture(str(path), host)
    assert _run("gpu", str(path)) == {"proofs": 128}
