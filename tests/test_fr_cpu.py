"""The BLS12-381 scalar field on the CPU (build/lb_fr_harness.so: the LB_HD code of lb_fr.h that the
k_fr_* kernels of lb_kzg_field.h run, compiled for x86) against Python integers and the host
field work of lodestar_amd/kzg.py: field operations, the radix-2 transform, the evaluate-and-divide
scan, and a stand-alone program of the same checks under the address and undefined-behaviour
sanitizers."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from lodestar_amd import kzg as K

R = K.BLS_MODULUS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGE = [0, 1, 2, R - 1, R - 2, (1 << 255) % R]
_rnd = random.Random(0xF7)
PAIRS = [(a, b) for a in EDGE for b in EDGE] + [(_rnd.randrange(R), _rnd.randrange(R)) for _ in range(200)]


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_fr_harness
    lib = ctypes.CDLL(build_fr_harness(verbose=False))
    c = ctypes.c_char_p
    lib.c_fr_op.argtypes = [ctypes.c_int, c, c, c]
    lib.c_fr_pow.argtypes = [c, c, c]
    lib.c_fr_from_be32.argtypes = [c, c]
    lib.c_fr_reduce256.argtypes = [c, c]
    lib.c_fr_ntt.argtypes = [ctypes.c_int, c, c]
    lib.c_fr_intt_brp.argtypes = [ctypes.c_int, c, ctypes.c_uint32]
    lib.c_fr_eval_quotient.argtypes = [ctypes.c_uint32, c, c, c, c]
    return lib


def le(v):
    return int(v).to_bytes(32, "little")


def vec(vals):
    return ctypes.create_string_buffer(b"".join(le(v) for v in vals), 32 * len(vals))


def unvec(buf, n):
    return [int.from_bytes(buf.raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def op(L, code, a, b=0):
    out = ctypes.create_string_buffer(32)
    L.c_fr_op(code, le(a), le(b), out)
    return int.from_bytes(out.raw, "little")


def test_field_operations(L):
    for a, b in PAIRS:
        assert op(L, 0, a, b) == a * b % R, (a, b)
        assert op(L, 1, a, b) == (a + b) % R, (a, b)
        assert op(L, 2, a, b) == (a - b) % R, (a, b)
        assert op(L, 3, a) == -a % R, a
        assert op(L, 5, a) == a * a % R, a
    for a in EDGE + [p[0] for p in PAIRS[-20:]]:
        inv = op(L, 4, a)
        assert inv == pow(a, R - 2, R), a
        assert a == 0 or inv * a % R == 1
    out = ctypes.create_string_buffer(32)
    for a, e in ((7, (R - 1) // 4096), (R - 1, 2 ** 256 - 1), (5, 0), (0, 0), (PAIRS[-1][0], PAIRS[-1][1])):
        L.c_fr_pow(le(a), le(e), out)
        assert int.from_bytes(out.raw, "little") == pow(a, e, R), (a, e)


def test_from_be32_reports_the_range(L):
    out = ctypes.create_string_buffer(32)
    for v, ok in ((0, 1), (1, 1), (R - 1, 1), (R, 0), (R + 1, 0), (2 ** 256 - 1, 0)):
        assert L.c_fr_from_be32(v.to_bytes(32, "big"), out) == ok, v
        assert int.from_bytes(out.raw, "little") == v % R, v


def test_reduce256(L):
    out = ctypes.create_string_buffer(32)
    for v in (0, R - 1, R, 2 * R - 1, 2 * R, 2 ** 256 - 1):
        L.c_fr_reduce256(le(v), out)
        assert int.from_bytes(out.raw, "little") == v % R, v


def _inputs(n, seed):
    rnd = random.Random(seed)
    unit = lambda k: [1 if i == k else 0 for i in range(n)]  # noqa: E731
    return [unit(0), unit(1), unit(n - 1), [R - 5] * n, [rnd.randrange(R) for _ in range(n)]]


@pytest.mark.parametrize("logn", [1, 2, 3, 6, 12])
def test_transform_matches_host_ntt(L, logn):
    """fr_ntt_bitrev + fr_ntt_stage against kzg.py _ntt, with the forward and the inverse roots"""
    n = 1 << logn
    w = pow(K.PRIMITIVE_ROOT_OF_UNITY, (R - 1) // n, R)
    for root in (w, pow(w, R - 2, R)):
        roots = [pow(root, k, R) for k in range(n)]
        for a in _inputs(n, 100 + logn):
            buf = vec(a)
            L.c_fr_ntt(logn, buf, le(root))
            assert unvec(buf, n) == K._ntt(list(a), roots), (logn, a[:4])


@pytest.mark.parametrize("logn", [1, 2, 3, 6, 12])
def test_inverse_transform_of_bit_reversed_evaluations(L, logn):
    """the kernel's form (no reversal, the fr_intt_table twiddles, times 1/n): coefficients of the
    polynomial whose values at the bit-reversed roots are given; at 4096 that is
    evaluations_to_coefficients, with the work split over 1 and over 1024 lanes"""
    n = 1 << logn
    w = pow(K.PRIMITIVE_ROOT_OF_UNITY, (R - 1) // n, R)
    brp = K._brp_index(n)
    inv_roots = [pow(w, (-k) % n, R) for k in range(n)]
    inv_n = pow(n, R - 2, R)
    for a in _inputs(n, 200 + logn):
        if n == K.FIELD_ELEMENTS_PER_BLOB:
            exp = K.evaluations_to_coefficients(a)
        else:
            nat = [0] * n
            for i, v in enumerate(a):
                nat[brp[i]] = v
            exp = [c * inv_n % R for c in K._ntt(nat, inv_roots)]
        for nthr in (1, 1024):
            buf = vec(a)
            L.c_fr_intt_brp(logn, buf, nthr)
            assert unvec(buf, n) == exp, (logn, nthr, a[:4])


@pytest.mark.parametrize("n", [8, 4096])
def test_evaluate_and_quotient(L, n):
    rnd = random.Random(300 + n)
    coeffs = [rnd.randrange(R) for _ in range(n)]
    buf = vec(coeffs)
    for z in (0, 1, R - 1, K.ROOTS_BRP[1], rnd.randrange(R)):
        q = ctypes.create_string_buffer(32 * n)
        y = ctypes.create_string_buffer(32)
        L.c_fr_eval_quotient(n, buf, le(z), q, y)
        got = unvec(q, n)
        assert got[:n - 1] == K.quotient_coefficients(coeffs, z), (n, z)
        assert got[n - 1] == 0
        assert int.from_bytes(y.raw, "little") == K.evaluate_coefficients(coeffs, z), (n, z)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_field_and_transform_under_sanitizers(tmp_path):
    """tests/native/fr_check.cpp: the field identities and the 4096-point transform round trip in a
    program of its own, built with -fsanitize=address,undefined"""
    exe = tmp_path / "fr_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "fr_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fr_check: failures 0" in out.stdout
