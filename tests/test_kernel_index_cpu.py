"""The index arithmetic that kernels of lb_kernels.h share (lodestar_amd/csrc/lb_kernel_index.h: the
digit split of the bucket MSM's count and scatter passes, the segment heads of a set's chunk sums) in
a stand-alone program on the CPU under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_msm_digits_and_segment_heads_under_sanitizers(tmp_path):
    """tests/native/kernel_index_check.cpp: msm_for_digits<4> and <6> recompose every weighted scalar
    half (weights 1 .. the kernels' LB_WT_MAX), skip zero digits and stay below W windows; the walk by
    seg_next_head and seg_is_head name exactly a set's first chunk and its chunks at multiples of 64,
    for every c0 <= c1 <= 200"""
    wt_max = re.search(r"^#define LB_WT_MAX (\d+) ", open(os.path.join(CSRC, "lb_kernels.h")).read(), re.M).group(1)
    exe = tmp_path / "kernel_index_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DLB_WT_MAX=" + wt_max, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "kernel_index_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kernel_index_check: failures 0" in out.stdout
