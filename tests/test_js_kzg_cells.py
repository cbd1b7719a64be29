"""tests/js/test_kzg_cells.js: the cell names (EIP-7594) of lodestar_amd/js/kzg.js.  Without a GPU:
argument validation and the batch combiner against Python.  On the GPU: computeCells gives the
Python transform's bytes and verifyCellKzgProofBatch(Many) the verdicts of the Python surface, over
fixture bytes written by tests/test_kzg_cells.py's helper."""
import json
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402

from lodestar_amd import kzg as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_kzg_cells.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")
R = K.BLS_MODULUS


def _run(*args):
    if NODE is None:
        pytest.skip("node not installed")
    if not os.path.exists(ADDON):
        from lodestar_amd.build import build_napi
        build_napi(verbose=False)
    r = subprocess.run([NODE, SCRIPT, *args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"js kzg cells {args[0]} ok", r.stdout
    return json.loads(lines[-2])


def test_js_combiner_matches_python():
    got = _run("cpu")
    cell = lambda v: bytes([v]) * 2048   # noqa: E731
    a, b, p = b"\x11" * 48, b"\x22" * 48, b"\x33" * 48
    cases = [([], [], [], []), ([a], [127], [cell(1)], [p]),
             ([a, b, p], [0, 64, 127], [cell(1), cell(2), cell(3)], [p, p, a]),
             ([b, a, b], [5, 5, 6], [cell(1), cell(2), cell(3)], [p, p, a])]
    assert [int(v) for v in got["r"]] == [K.compute_cell_batch_r(*c) for c in cases] == [S.compute_cell_batch_r(*c) for c in cases]


@pytest.mark.gpu
def test_js_names_match_the_python_surface(engine, tmp_path):
    import test_kzg_cells as T
    host = K.Kzg(engine)
    comms = [host.g1_lincomb(c) for c in T.COEFFS]
    pairs = T.PAIRS[1:4]
    fx = {"comms": comms, "c": [None] + [comms[b] for b, _ in pairs], "i": [None] + [i for _, i in pairs],
          "cells": [None] + [T.CELLS[b][i] for b, i in pairs],
          "p": [None] + [host.g1_lincomb(S.cell_quotient(T.COEFFS[b], i)[0]) for b, i in pairs]}
    path = tmp_path / "cells.json"
    T.write_js_fixture(str(path), host, fx)
    got = _run("gpu", str(path))
    c, i, x, p = fx["c"][1:], fx["i"][1:], fx["cells"][1:], fx["p"][1:]
    elem_r = R.to_bytes(32, "big") + x[0][32:]
    flagless = bytes([p[1][0] & 0x7F]) + p[1][1:]
    groups = [(c, i, x, p), ([], [], [], []), (c, i, x, [p[1], p[0], p[2]]), (c, i, [elem_r] + x[1:], p),
              (c, i, x, [p[0], flagless, p[2]]), (c[1:], i[1:], x[1:], p[1:])]
    exp = [f"Error: {str(v).split(': ', 1)[1]}" if isinstance(v, K.KzgError) else v
           for v in host.verify_cell_kzg_proof_batch_many(groups)]
    assert got["many"] == exp
    assert exp[:3] == [True, True, False] and exp[3] == "Error: BLST_BAD_SCALAR" and exp[4].startswith("Error: ") and exp[5] is True
    assert got["single"] == [True, True, False]
