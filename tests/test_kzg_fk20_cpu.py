"""FK20 (lb_kzg_compute_cells_and_proofs) on the CPU: the pure-Python restatement
tests/kzg_fk20_spec.py against the definition of a cell proof (tests/kzg_cells_spec.py's long
division) in the scalar model, where the setup "points" are tau^t for a known tau; then
build/lb_kzg_fk20_harness.so -- the column gather and transforms of k_fr_fk_cols and the stage
schedule of k_g1_fft128, compiled for x86 -- against that restatement, the schedule over the scalar
field against a plain recursive transform and over real G1 points against the oracle; and a
stand-alone program of the same cases under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
import kzg_fk20_spec as F  # noqa: E402

from oracle import bls_oracle as o  # noqa: E402

R = S.R
N = S.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RND = random.Random(0xF20)
TAU = RND.randrange(R)
SETUP = [pow(TAU, t, R) for t in range(N)]                      # the scalar model: s[t] = tau^t
DENSE = [RND.randrange(R) for _ in range(N)]
POLYS = {"dense": DENSE, "degree 70": [RND.randrange(1, R) for _ in range(71)], "degree 64": [RND.randrange(1, R) for _ in range(65)],
         "degree 63": [RND.randrange(1, R) for _ in range(64)], "X^4095": [0] * 4095 + [1]}
CELLS_CHECKED = [0, 1, 5, 63, 64, 127]


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_kzg_fk20_harness
    lib = ctypes.CDLL(build_kzg_fk20_harness(verbose=False))
    c, u, i = ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int
    lib.c_fk_cols.argtypes = [c, c]
    lib.c_fk_fft_fr.argtypes = [c, u, i, i, c]
    lib.c_fk_fft_g1.argtypes = [ctypes.POINTER(ctypes.c_uint64), u, i, i, c, ctypes.POINTER(ctypes.c_int32)]
    lib.c_fk_setup_index.argtypes = [u, u]
    lib.c_fk_setup_index.restype = u
    lib.c_fk_col_index.argtypes = [u, u]
    lib.c_fk_col_index.restype = u
    return lib


def _le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _from_le(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


@pytest.mark.parametrize("name", list(POLYS))
def test_spec_gives_the_commitment_of_the_long_division_quotient(name):
    coeffs = POLYS[name]
    got = F.proofs(coeffs, SETUP)
    for i in CELLS_CHECKED:
        q, _ = S.cell_quotient(coeffs, i)
        assert got[i] == sum(qu * SETUP[u] for u, qu in enumerate(q)) % R, (name, i)


def test_spec_toeplitz_rows_and_the_upper_half_that_must_be_zeroed():
    h = F.toeplitz(DENSE, SETUP)
    assert h[:63] == [F.h_direct(DENSE, SETUP, j) for j in range(63)]
    assert h[63] == 0
    assert any(h[64:])                                            # without the zeroing step the proofs would be wrong
    unzeroed = F.dft(h)
    assert unzeroed[S.brp(5, 7)] != F.proofs(DENSE, SETUP)[5]


def test_index_maps_match_the_spec(L):
    s = list(range(1, N + 1))                                     # "points" that name their own index
    for i in (0, 1, 62, 63):
        col = F.setup_column(s, i)
        assert [L.c_fk_setup_index(i, j) for j in range(128)] == [v - 1 if v else 0xFFFFFFFF for v in col]
        bcol = F.blob_column(s, i)
        assert [L.c_fk_col_index(i, k) for k in range(128)] == [v - 1 if v else 0xFFFFFFFF for v in bcol]


@pytest.mark.parametrize("name,coeffs", [("dense", DENSE), ("X^64", [0] * 64 + [1]), ("X^4095", [0] * 4095 + [1]),
                                         ("X^63", [0] * 63 + [1])])
def test_column_transforms_equal_the_spec(L, name, coeffs):
    out = ctypes.create_string_buffer(32 * 8192)
    L.c_fk_cols(_le(list(coeffs) + [0] * (N - len(coeffs))), out)
    got = _from_le(out.raw, 8192)
    cs = F.column_transforms(coeffs)
    assert got == [cs[e % 64][e // 64] * F.INV_128 % R for e in range(8192)]
    if name == "X^63":
        assert not any(got)                                       # below X^64 nothing reaches a proof


def _fft_fr(L, vals, n_live=128, inverse=False, scale=False):
    out = ctypes.create_string_buffer(32 * 128)
    L.c_fk_fft_fr(_le(vals), n_live, int(inverse), int(scale), out)
    return _from_le(out.raw, 128)


def test_stage_schedule_over_the_scalar_field(L):
    v = [RND.randrange(R) for _ in range(128)]
    fwd = S._fft(v, F.W128)
    assert _fft_fr(L, v) == fwd
    assert _fft_fr(L, v, inverse=True, scale=True) == F.dft(v, inverse=True)
    assert _fft_fr(L, v, inverse=True) == S._fft(v, F.W128_INV)   # unscaled: the pipeline folds 1 / 128 into the scalars
    assert _fft_fr(L, fwd, inverse=True, scale=True) == v
    assert _fft_fr(L, v, n_live=64) == S._fft(v[:64] + [0] * 64, F.W128)
    one_hot = [0] * 128
    one_hot[1] = 1
    assert _fft_fr(L, one_hot) == [pow(F.W128, m, R) for m in range(128)]


def test_stage_schedule_over_g1_points(L):
    """input j = [k_j] G with small known k_j, some at infinity: output m must be [sum k_j w128^(j m)] G"""
    ks = [RND.randrange(1, 1 << 20) for _ in range(128)]
    for j in (0, 7, 64, 100, 127):
        ks[j] = 0
    arr = (ctypes.c_uint64 * 128)(*ks)
    out = ctypes.create_string_buffer(96 * 128)
    inf = (ctypes.c_int32 * 128)()
    L.c_fk_fft_g1(arr, 128, 0, 0, out, inf)
    want = S._fft(ks, F.W128)
    for m in (0, 1, 64, 127):
        x, y = int.from_bytes(out.raw[96 * m: 96 * m + 48], "big"), int.from_bytes(out.raw[96 * m + 48: 96 * m + 96], "big")
        assert inf[m] == 0 and (x, y) == o.g1_mul(o.G1, want[m]), m
    # all-infinity input stays infinity; the inverse transform with its scale, of one point among infinities
    L.c_fk_fft_g1((ctypes.c_uint64 * 128)(), 128, 0, 0, out, inf)
    assert list(inf) == [1] * 128
    spike = [0] * 128
    spike[3] = 5
    L.c_fk_fft_g1((ctypes.c_uint64 * 128)(*spike), 128, 1, 1, out, inf)
    want = F.dft(spike, inverse=True)
    for m in (0, 5):
        x, y = int.from_bytes(out.raw[96 * m: 96 * m + 48], "big"), int.from_bytes(out.raw[96 * m + 48: 96 * m + 96], "big")
        assert inf[m] == 0 and (x, y) == o.g1_mul(o.G1, want[m])


def test_fk20_pieces_under_sanitizers(tmp_path):
    """tests/native/kzg_fk20_check.cpp: the harness cases in a program of its own, built with
    -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "kzg_fk20_check"
    subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "harness"),
                    os.path.join(ROOT, "tests", "native", "kzg_fk20_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kzg_fk20_check: failures 0" in out.stdout
