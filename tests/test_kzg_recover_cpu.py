"""Cell recovery (lb_kzg_recover_cells_and_proofs) on the CPU: the big-integer helper
tests/kzg_recover_spec.py -- the consensus spec's route taken literally and the column route the
kernels run -- against the original coefficients; then build/lb_kzg_recover_harness.so, the lane
functions of lb_recover.h compiled for x86 with the kernels' addressing, against that helper; and a
stand-alone program of the same cases under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_cells_spec as S  # noqa: E402
import kzg_recover_spec as V  # noqa: E402

R = S.R
N = S.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RND = random.Random(0x7EC0)
POLYS = {"dense": [RND.randrange(R) for _ in range(N)], "degree 70": [RND.randrange(1, R) for _ in range(71)],
         "X^4095": [0] * 4095 + [1], "constant": [RND.randrange(1, R)], "zero": []}
INDEX_SETS = {"0..63": list(range(64)), "64..127": list(range(64, 128)), "evens": list(range(0, 128, 2)),
              "odds": list(range(1, 128, 2)), "random 64": sorted(random.Random(64).sample(range(128), 64)),
              "random 65": sorted(random.Random(65).sample(range(128), 65)), "all but 0": list(range(1, 128)),
              "all but 127": list(range(127)), "all 128": list(range(128))}
CELLS = {name: V.cells_of(p) for name, p in POLYS.items()}      # computed once, never changed
CASES = [(p, s) for p in POLYS for s in INDEX_SETS]


def _padded(coeffs):
    return list(coeffs) + [0] * (N - len(coeffs))


def _given(poly, idx):
    return [CELLS[poly][i] for i in idx]


def _changed(poly, idx, which=3, elem=17):
    """the given cells with one value changed"""
    cells = [list(c) for c in _given(poly, idx)]
    cells[which][elem] = (cells[which][elem] + 1) % R
    return cells


def test_fast_interpolation_is_the_definition():
    for i in (0, 5, 127):
        assert V.interpolate(i, CELLS["dense"][i]) == S.interpolate(i, CELLS["dense"][i])


@pytest.mark.parametrize("poly,iset", CASES)
def test_both_routes_return_the_coefficients(poly, iset):
    idx = INDEX_SETS[iset]
    want = _padded(POLYS[poly])
    assert V.recover_spec(idx, _given(poly, idx)) == want
    coeffs, upper = V.recover_columns(idx, _given(poly, idx))
    assert coeffs == want
    assert not any(any(u) for u in upper)


def test_a_changed_value_among_65_cells_shows_in_an_upper_half():
    idx = INDEX_SETS["random 65"]
    _, upper = V.recover_columns(idx, _changed("dense", idx))
    assert any(any(u) for u in upper)


def test_a_changed_value_among_64_cells_is_another_polynomial():
    idx = INDEX_SETS["random 64"]
    cells = _changed("dense", idx)
    coeffs, upper = V.recover_columns(idx, cells)
    assert not any(any(u) for u in upper)
    assert coeffs != _padded(POLYS["dense"])
    got = V.cells_of(coeffs)
    assert [got[i] for i in idx] == cells


# ------------------------------------------------------------------ the x86 harness of lb_recover.h
@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_kzg_recover_harness
    lib = ctypes.CDLL(build_kzg_recover_harness(verbose=False))
    c, u = ctypes.c_char_p, ctypes.c_uint32
    u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    for name, args in {"c_rc_point": [u], "c_rc_slot": [u], "c_rc_rank": [u32p, u], "c_rc_coef_index": [u, u]}.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = u
    lib.c_rc_plan.argtypes = [u, u32p, u32p, u32p]
    lib.c_rc_zero.argtypes = [u32p, c, c]
    lib.c_rc_recover.argtypes = [u, u32p, c, c, c, i32p]
    lib.c_rc_blob.argtypes = [c, u, c]
    return lib


def _le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _from_le(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def _u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def _mask(idx):
    m = [0, 0, 0, 0]
    for i in idx:
        m[i >> 5] |= 1 << (i & 31)
    return m


def _harness_recover(L, idx, cells):
    """(rc, coefficients, upper halves as the helper states them, flags)"""
    interp = V.interpolated(idx, cells)
    coef, upper = ctypes.create_string_buffer(32 * N), ctypes.create_string_buffer(32 * 64 * 64)
    flags = (ctypes.c_int32 * 64)()
    rc = L.c_rc_recover(len(idx), _u32(idx), _le([c for cell in interp for c in cell]), coef, upper, flags)
    # the harness shows slots 64 .. 127 as the last transform leaves them: Q[k] s^k 128^2
    unscale = [pow(V.inv(V.SHIFT), k, R) * V.inv(128 * 128) % R for k in range(64, 128)]
    raw = _from_le(upper.raw, 64 * 64)
    ups = [[raw[64 * r + k] * unscale[k] % R for k in range(64)] for r in range(64)]
    return rc, _from_le(coef.raw, N), ups, list(flags)


def test_slot_map_rank_and_write_back_index(L):
    for i in range(128):
        assert L.c_rc_point(i) == V.point(i) == S.brp(i, 7)
        assert L.c_rc_slot(i) == S.brp(V.point(i), 7) == i           # the load's reversal undoes the point's
    for name in ("random 64", "random 65", "all but 0", "odds"):
        idx = INDEX_SETS[name]
        m = _u32(_mask(idx))
        assert [L.c_rc_rank(m, i) for i in idx] == list(range(len(idx)))
        assert L.c_rc_rank(m, 127) == len([i for i in idx if i < 127])
    assert sorted(L.c_rc_coef_index(k, r) for k in range(64) for r in range(64)) == list(range(N))
    assert [L.c_rc_coef_index(k, r) for k, r in ((0, 0), (0, 63), (1, 0), (63, 63))] == [0, 63, 64, 4095]


@pytest.mark.parametrize("n_missing", [0, 1, 63, 64])
def test_vanishing_values(L, n_missing):
    missing = set(random.Random(n_missing).sample(range(128), n_missing))
    idx = [i for i in range(128) if i not in missing]
    zev, zcinv = ctypes.create_string_buffer(32 * 128), ctypes.create_string_buffer(32 * 128)
    L.c_rc_zero(_u32(_mask(idx)), zev, zcinv)
    want_zev, want_zcinv = V.zero_values(idx)
    assert _from_le(zev.raw, 128) == want_zev
    assert _from_le(zcinv.raw, 128) == want_zcinv
    assert [m for m, z in enumerate(want_zev) if z == 0] == sorted(V.point(i) for i in missing)


@pytest.mark.parametrize("poly,iset", CASES)
def test_column_pipeline_equals_the_helper(L, poly, iset):
    idx = INDEX_SETS[iset]
    rc, coeffs, upper, flags = _harness_recover(L, idx, _given(poly, idx))
    assert rc == 0
    assert coeffs == _padded(POLYS[poly])
    assert not any(flags) and not any(any(u) for u in upper)


def test_inconsistency_flag(L):
    idx = INDEX_SETS["random 65"]
    cells = _changed("dense", idx)
    rc, coeffs, upper, flags = _harness_recover(L, idx, cells)
    want_coeffs, want_upper = V.recover_columns(idx, cells)
    assert rc == 0 and coeffs == want_coeffs and upper == want_upper
    assert flags == [int(any(u)) for u in want_upper] and any(flags)
    idx = INDEX_SETS["random 64"]
    cells = _changed("dense", idx)
    rc, coeffs, upper, flags = _harness_recover(L, idx, cells)
    assert rc == 0 and not any(flags)
    assert coeffs == V.recover_columns(idx, cells)[0]


def test_argument_check(L):
    def plan(groups):
        off = [0]
        for g in groups:
            off.append(off[-1] + len(g))
        flat = [i for g in groups for i in g] or [0]
        mask = (ctypes.c_uint32 * (4 * len(groups)))()
        return L.c_rc_plan(len(groups), _u32(off), _u32(flat), mask), list(mask)

    ok, mask = plan([INDEX_SETS["random 64"], list(range(128)), INDEX_SETS["odds"]])
    assert ok == 1
    assert mask == _mask(INDEX_SETS["random 64"]) + [0xFFFFFFFF] * 4 + [0xAAAAAAAA] * 4
    assert plan([list(range(63))])[0] == 0
    assert plan([list(range(128)) + [128]])[0] == 0                    # 129 cells
    assert plan([list(range(63)) + [128]])[0] == 0                     # an index past the last cell
    assert plan([list(range(63)) + [62]])[0] == 0                      # a duplicate
    assert plan([[1, 0] + list(range(2, 64))])[0] == 0                 # a descending pair
    assert plan([list(range(64)), list(range(63))])[0] == 0            # the second blob is short
    bad_off = _u32([1, 65])
    assert L.c_rc_plan(1, bad_off, _u32(list(range(65))), (ctypes.c_uint32 * 4)()) == 0
    assert L.c_rc_plan(2, _u32([0, 64, 0]), _u32(list(range(64))), (ctypes.c_uint32 * 8)()) == 0


@pytest.mark.parametrize("nthr", [1024, 64])
def test_blob_elements_from_coefficients(L, nthr):
    for name in ("dense", "degree 70", "zero"):
        out = ctypes.create_string_buffer(32 * N)
        L.c_rc_blob(_le(_padded(POLYS[name])), nthr, out)
        assert S.values_to_blob(_from_le(out.raw, N)) == S.coefficients_to_blob(POLYS[name])


def test_recover_pieces_under_sanitizers(tmp_path):
    """tests/native/kzg_recover_check.cpp: the harness cases in a program of its own, built with
    -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "kzg_recover_check"
    subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "harness"),
                    os.path.join(ROOT, "tests", "native", "kzg_recover_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kzg_recover_check: failures 0" in out.stdout
