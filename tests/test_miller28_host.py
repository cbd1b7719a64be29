"""The limb-resident per-root Miller loop (lb_field.h fp6_28; lb_pairing.h miller_dbl28, miller_add28,
f_sqr28, f_line28, miller_lane28: the loop k_miller_lane runs) against miller_loop_inl on the host:
tests/native/miller28_check.cpp built from the device headers with -DLB_FP28_CHECK, which makes every
product assert its 64-bit columns against 128-bit sums and makes the layer propagate worst-case limb
and value bounds from the loop invariant, re-assumed at the top of every step and before every
addition pass, aborting where one fails.  A clean exit therefore means: all 144 canonical words equal
for every pair of tests/golden/miller28_pairs.txt (random P in G1 and Q in G2, the generators,
P = (0, 2), a coordinate of P equal to p - 1), and no bound fired.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(ROOT, "tests", "golden", "miller28_pairs.txt")


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-DLB_FP28_CHECK", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "miller28_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), PAIRS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pairs: 12 " in out.stdout and "failures: 0" in out.stdout, out.stdout
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_miller28_loop_matches_with_bounds_asserted(tmp_path):
    _build_and_run(tmp_path, "miller28_check", [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_miller28_same_vectors_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program itself, instrumented; nothing is loaded into python"""
    out = _build_and_run(tmp_path, "miller28_check_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_golden_pairs_are_what_the_generator_writes():
    """tests/golden/miller28_pairs.txt is tools/gen_miller28_vectors.py's output"""
    import contextlib
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location("gen_miller28_vectors",
                                                  os.path.join(ROOT, "tools", "gen_miller28_vectors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        gen.main()
    with open(PAIRS) as f:
        assert f.read() == buf.getvalue()
