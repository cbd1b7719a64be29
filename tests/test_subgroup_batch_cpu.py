"""The per-batch signature subgroup test on the host: tests/native/subgroup_batch_check.cpp,
built from the device headers with g++.

1. The selection (lb_pipeline_plan.h pipe_plan_subgroup_batch) on every point of its grid, S-sum form x
   scalars given x enabled, against the rule written out here: only the bucket MSM, only scalars the engine
   draws, only while enabled.
2. The mixing (lb_curve.h g2_mix_share, a lane's share in k_subgroup_mix, and the sum of the shares) and
   Scott's test over 16 buckets and 64 tests filled from tests/golden/subgroup28_points.txt.  The program
   checks every single test against what the picked buckets' torsion parts give; this file checks the batch
   verdict of each case against the table below.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = os.path.join(ROOT, "tests", "golden", "subgroup28_points.txt")
SSUM_BUCKET_MSM = 4  # lb_pipeline_plan.h ssum_form: PAR_W4, UNBLINDED, TERMS_G8, TERMS_LANE, BUCKET_MSM

# the batch verdict of each case: all-G2 buckets pass; a bucket with an order-13 / order-23 / large-cofactor
# / mixed component fails; T and -T in two buckets fail; T + (-T) inside one bucket is clean and passes; the
# same small-order point twice fails, thirteen times an order-13 point is clean
CASES = {
    "all_g2": "pass", "one_ord13": "fail", "one_ord23": "fail", "one_curve": "fail", "one_mixed": "fail",
    "lone_ord13": "fail", "pair_ord13": "fail", "pair_curve": "fail", "cancel_in_bucket": "pass",
    "twice_ord23": "fail", "thirteen_ord13": "pass",
}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "subgroup_batch_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), POINTS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "points: 22 " in out.stdout and "failures: 0" in out.stdout, out.stdout
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("sgb"), "subgroup_batch_check", [])


def test_selection_over_its_grid(run):
    got = {}
    for line in run.stdout.splitlines():
        if line.startswith("plan "):
            ss, given, en, v = (int(x) for x in line.split()[1:])
            got[(ss, given, en)] = v
    want = {(ss, given, en): int(ss == SSUM_BUCKET_MSM and not given and en)
            for ss in range(5) for given in (0, 1) for en in (0, 1)}
    assert got == want
    assert sum(want.values()) == 1


def test_mixing_and_test_verdicts(run):
    got = {}
    for line in run.stdout.splitlines():
        if line.startswith("case "):
            _, name, verdict, agree = line.split()
            assert agree == "ok", line  # every one of the 64 tests gave what its picked buckets determine
            got[name] = verdict
    assert got == CASES


def test_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program itself, instrumented; nothing is loaded into python"""
    out = _build_and_run(tmp_path, "subgroup_batch_check_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
