"""The resident pubkey table's fixed-base comb on the CPU (build/lb_comb_harness.so: the LB_HD code
of lb_curve.h that k_comb_fill and k_pk_blind_comb run, compiled for x86): one key's 72-entry table
built on the host, comb(P, w) against the GLV ladder jac_mul_glv(P, w) that k_pk_blind runs, after
affine conversion, and against the oracle's [lo + hi lambda]P."""
import ctypes
import random

import pytest

from oracle import bls_oracle as o

# the issue's words: 1 and 2, all ones, every digit carrying, hi only, lo only
WORDS = [1, 2, 0xFFFFFFFFFFFFFFFF, 0x8888888888888888, 0x0000000100000000, 0x00000000FFFFFFFF]
_rnd = random.Random(0xC0B)
WORDS += [_rnd.getrandbits(64) or 1 for _ in range(64)]  # ... and 64 seeded random words


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_comb_harness
    lib = ctypes.CDLL(build_comb_harness(verbose=False))
    lib.c_comb_digits.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]
    lib.c_comb_mul.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    lib.c_glv_mul.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    return lib


def g1b(pt):
    return (pt[0] % o.P).to_bytes(48, "big") + (pt[1] % o.P).to_bytes(48, "big")


def fg1(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def keys():
    r = random.Random(77)
    return [o.G1] + [o.g1_mul(o.G1, r.randrange(1, o.R)) for _ in range(2)]


def table_of(L, pt):
    t = ctypes.create_string_buffer(L.c_comb_entries() * L.c_comb_entry_bytes())
    L.c_comb_build(g1b(pt), t)
    return t


def test_layout(L):
    assert L.c_comb_entries() == 72 and L.c_comb_entry_bytes() == 96


def test_recoding(L):
    """h = sum d_j 16^j with d_j in [-8, 8] for both halves of every word; the entry read is
    8 j + |d| - 1; 0x88888888 carries out of every digit."""
    d = (ctypes.c_int32 * 18)()
    e = (ctypes.c_uint32 * 18)()
    for w in WORDS + [0x0000000800000007, 0x7777777780000000]:
        L.c_comb_digits(w, d, e)
        for half, h in ((0, w & 0xFFFFFFFF), (1, w >> 32)):
            ds = [d[9 * half + j] for j in range(9)]
            assert all(-8 <= x <= 8 for x in ds)
            assert sum(x * 16**j for j, x in enumerate(ds)) == h
            for j, x in enumerate(ds):
                assert e[9 * half + j] == 8 * j + (abs(x) - 1 if x else 0)
    L.c_comb_digits(0x8888888888888888, d, e)
    assert [d[j] for j in range(9)] == [-8] + [-7] * 7 + [1]


@pytest.mark.parametrize("k", range(3))
def test_comb_equals_glv_ladder(L, k):
    pt = keys()[k]
    t = table_of(L, pt)
    out_c, out_g = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    for w in WORDS:
        ok_c = L.c_comb_mul(t, w, out_c)
        ok_g = L.c_glv_mul(g1b(pt), w, out_g)
        assert ok_c == ok_g == 1, hex(w)
        assert out_c.raw == out_g.raw, hex(w)
    # ... and the oracle's own scalar multiplication for a few of them (slow in Python)
    for w in WORDS[:6] + WORDS[6:10]:
        L.c_comb_mul(t, w, out_c)
        assert fg1(out_c.raw) == o.g1_mul(pt, o.blinding_scalar(w)), hex(w)


def test_small_order_key(L):
    """An unvalidated key may be a curve point outside G1: (0, 2) has order 3, so a third of its
    entries are at infinity (stored as zeros and skipped).  Comb and ladder still agree, the
    point at infinity included."""
    pt = (0, 2)
    assert o.g1_on_curve(pt)
    t = table_of(L, pt)
    assert t.raw[96 * 2:96 * 3] == bytes(96)  # [3]P
    out_c, out_g = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    for w in WORDS[:24]:
        ok_c = L.c_comb_mul(t, w, out_c)
        ok_g = L.c_glv_mul(g1b(pt), w, out_g)
        assert ok_c == ok_g, hex(w)
        if ok_c:
            assert out_c.raw == out_g.raw, hex(w)
