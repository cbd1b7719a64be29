"""The per-lane pieces of the batched KZG verification on the CPU (build/lb_kzg_batch_harness.so:
the LB_HD code of lb_fr.h that k_fr_aggregate_seg and k_fr_eval_many run, compiled for x86) against
Python integers: the segmented aggregation, the evaluation of 4096-coefficient polynomials, and a
stand-alone program of the same cases under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from lodestar_amd import kzg as K

R = K.BLS_MODULUS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = K.FIELD_ELEMENTS_PER_BLOB


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_kzg_batch_harness
    lib = ctypes.CDLL(build_kzg_batch_harness(verbose=False))
    c = ctypes.c_char_p
    lib.c_fr_aggregate_seg.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, c, c, c]
    lib.c_fr_eval.argtypes = [ctypes.c_uint32, c, c, c]
    return lib


def le(v):
    return int(v).to_bytes(32, "little")


def vec(vals):
    return ctypes.create_string_buffer(b"".join(le(v) for v in vals), 32 * len(vals))


def unvec(buf, n):
    return [int.from_bytes(buf.raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def test_segmented_aggregation(L):
    """sidecars of 0, 1, 2, 0 and 1 polynomials: each aggregate is its own polynomials' weighted sum,
    an empty sidecar's the zero polynomial"""
    offsets = [0, 0, 1, 3, 3, 4]
    n, length = len(offsets) - 1, 96
    rnd = random.Random(0xB47C)
    polys = [[rnd.randrange(R) for _ in range(length)] for _ in range(offsets[-1])]
    polys[1][0], polys[1][1], polys[2][2] = R - 1, 0, R - 1     # edge values inside the two-blob sidecar
    pw = [1, 1, rnd.randrange(R), 1]                            # r_k^j: 1, then r for the second of a sidecar
    off = np.asarray(offsets, np.uint32)
    out = ctypes.create_string_buffer(32 * n * length)
    L.c_fr_aggregate_seg(n, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), length,
                         vec([v for p in polys for v in p]), vec(pw), out)
    got = unvec(out, n * length)
    for k in range(n):
        exp = [sum(pw[j] * polys[j][i] for j in range(offsets[k], offsets[k + 1])) % R for i in range(length)]
        assert got[k * length: (k + 1) * length] == exp, k
    assert got[:length] == [0] * length == got[3 * length: 4 * length]


def _polys():
    rnd = random.Random(0xE7A1)
    last = [0] * N
    last[N - 1] = rnd.randrange(1, R)
    return {"random": [rnd.randrange(R) for _ in range(N)], "zero": [0] * N, "last": last}, rnd.randrange(R)


POLYS, Z_RANDOM = _polys()
POINTS = {"random": Z_RANDOM, "zero": 0, "one": 1, "root": K.ROOTS_BRP[5]}


@pytest.mark.parametrize("poly", sorted(POLYS))
@pytest.mark.parametrize("point", sorted(POINTS))
def test_evaluation_of_4096_coefficients(L, poly, point):
    """fr_eq_local, then the ten fr_ev_fold steps with fr_ev_weight, against Horner in Python integers"""
    coeffs, z = POLYS[poly], POINTS[point]
    y = ctypes.create_string_buffer(32)
    L.c_fr_eval(N, vec(coeffs), le(z), y)
    assert int.from_bytes(y.raw, "little") == K.evaluate_coefficients(coeffs, z), (poly, point)


def test_evaluation_of_a_short_polynomial(L):
    """8 coefficients: two lanes, one fold step"""
    rnd = random.Random(5)
    coeffs = [rnd.randrange(R) for _ in range(8)]
    for z in (0, 1, R - 1, rnd.randrange(R)):
        y = ctypes.create_string_buffer(32)
        L.c_fr_eval(8, vec(coeffs), le(z), y)
        assert int.from_bytes(y.raw, "little") == K.evaluate_coefficients(coeffs, z), z


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_batch_pieces_under_sanitizers(tmp_path):
    """tests/native/kzg_batch_check.cpp: the same cases in a program of its own, built with
    -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "kzg_batch_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "kzg_batch_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kzg_batch_check: failures 0" in out.stdout
