"""The limb-resident Fp2 layer (lb_field.h fp2_28) and the psi-ladder on it (lb_curve.h
g2_dbl_lean28, g2_madd_lean28, g2_aff_in_subgroup28) against the 12 x 32-bit forms, on the host:
tests/native/fp2_28_check.cpp built from the device headers with -DLB_FP28_CHECK, which makes every
product assert its 64-bit columns against 128-bit sums and makes the layer propagate worst-case limb
and value bounds through the ladder's formulas, aborting where one fails.  A clean exit therefore
means: equal results, equal verdicts on tests/golden/subgroup28_points.txt (points of G2, curve
points outside it, the small-order points, sums of both), and no bound fired.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = os.path.join(ROOT, "tests", "golden", "subgroup28_points.txt")


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-DLB_FP28_CHECK", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "fp2_28_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), POINTS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "points: 22 " in out.stdout and "failures: 0" in out.stdout, out.stdout
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_fp2_28_layer_and_ladder_match_with_bounds_asserted(tmp_path):
    _build_and_run(tmp_path, "fp2_28_check", [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_fp2_28_same_vectors_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program itself, instrumented; nothing is loaded into python"""
    out = _build_and_run(tmp_path, "fp2_28_check_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_golden_points_are_what_the_generator_writes():
    """tests/golden/subgroup28_points.txt is tools/gen_subgroup28_vectors.py's output (the oracle's
    points; the generator also checks that no curve point reaches the acc == +P addition)"""
    import contextlib
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location("gen_subgroup28_vectors",
                                                  os.path.join(ROOT, "tools", "gen_subgroup28_vectors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        gen.main()
    with open(POINTS) as f:
        assert f.read() == buf.getvalue()
