"""The host and per-lane pieces of the per-blob (Deneb) KZG calls on the CPU
(build/lb_kzg_blob_harness.so: lb_kzg_transcript.h's two transcripts, the phases of
k_fr_eval_quotient_many, the status fold of k_kzg_check_groups and lb_kzg_host.h's offsets
validator and per-item status fold, compiled for x86) against hashlib and Python integers; lodestar_amd.kzg's restatement of the transcripts against the independent one
of tests/kzg_deneb_spec.py; one low-degree proof through the pure-Python pairing; and a stand-alone
program of the harness cases under the address and undefined-behaviour sanitizers."""
import ctypes
import hashlib
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_deneb_spec as S  # noqa: E402

from lodestar_amd import _native as NAT  # noqa: E402
from lodestar_amd import kzg as K  # noqa: E402

R = S.R
N = S.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = ctypes.POINTER(ctypes.c_int32)
OK, BAD_SCALAR, NOT_IN_GROUP, BAD_ENCODING = NAT.LB_OK, NAT.LB_BAD_SCALAR, NAT.LB_POINT_NOT_IN_GROUP, 1


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_kzg_blob_harness
    lib = ctypes.CDLL(build_kzg_blob_harness(verbose=False))
    c, u = ctypes.c_char_p, ctypes.c_uint32
    lib.c_kzg_blob_challenge.argtypes = [c, c, c]
    lib.c_kzg_blob_challenges.argtypes = [u, c, c, u, c]
    lib.c_kzg_batch_r.argtypes = [u, c, c, c, c, c]
    lib.c_fr_eval_quotient_many.argtypes = [u, u, c, c, c, c]
    lib.c_kzg_group_status.argtypes = [I32, I32, u, u, u]
    lib.c_kzg_group_status.restype = ctypes.c_int32
    lib.c_kzg_offsets_ok.argtypes = [u, ctypes.POINTER(u), u]
    lib.c_kzg_offsets_ok.restype = ctypes.c_int32
    lib.c_kzg_fold_status.argtypes = [u, I32, I32, I32, c, u, c, u]
    return lib


def _random_blob(rnd):
    return b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(N))


def _hashlib_challenge(blob, c48):
    d = hashlib.sha256(b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big") + blob + c48).digest()
    return int.from_bytes(d, "big") % R


def _hashlib_r(cs, zs, ys, ps):
    data = b"RCKZGBATCH___V1_" + (4096).to_bytes(8, "big") + len(cs).to_bytes(8, "big")
    for c, z, y, p in zip(cs, zs, ys, ps):
        data += c + z.to_bytes(32, "big") + y.to_bytes(32, "big") + p
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R


RND = random.Random(0xDE9EB)
BLOBS = [_random_blob(RND) for _ in range(5)]
COMMS = [bytes(RND.randrange(256) for _ in range(48)) for _ in range(5)]   # the transcript takes any 48 bytes
PROOFS = [bytes(RND.randrange(256) for _ in range(48)) for _ in range(5)]


@pytest.mark.parametrize("blob", ["random", "zero"])
def test_blob_challenge_equals_hashlib(L, blob):
    b = BLOBS[0] if blob == "random" else bytes(32 * N)
    out = ctypes.create_string_buffer(32)
    L.c_kzg_blob_challenge(b, COMMS[0], out)
    exp = _hashlib_challenge(b, COMMS[0])
    assert int.from_bytes(out.raw, "big") == exp
    assert K.compute_challenge(b, COMMS[0]) == exp == S.compute_challenge(b, COMMS[0])


@pytest.mark.parametrize("n", [0, 1, 3])
def test_batch_r_equals_hashlib(L, n):
    rnd = random.Random(n)
    zs = [rnd.randrange(R) for _ in range(n)]
    ys = [0, R - 1, rnd.randrange(R)][:n]
    out = ctypes.create_string_buffer(32)
    be = lambda vs: b"".join(v.to_bytes(32, "big") for v in vs) or b"\x00"   # noqa: E731
    L.c_kzg_batch_r(n, b"".join(COMMS[:n]) or b"\x00", be(zs), be(ys), b"".join(PROOFS[:n]) or b"\x00", out)
    exp = _hashlib_r(COMMS[:n], zs, ys, PROOFS[:n])
    assert int.from_bytes(out.raw, "big") == exp
    assert K.compute_batch_r(COMMS[:n], zs, ys, PROOFS[:n]) == exp == S.compute_batch_r(COMMS[:n], zs, ys, PROOFS[:n])


def test_threaded_hashing_equals_single_thread(L):
    single = ctypes.create_string_buffer(32 * 5)
    L.c_kzg_blob_challenges(5, b"".join(BLOBS), b"".join(COMMS), 1, single)
    assert [int.from_bytes(single.raw[32 * i: 32 * i + 32], "big") for i in range(5)] == \
        [_hashlib_challenge(b, c) for b, c in zip(BLOBS, COMMS)]
    for threads in (2, 3, 8, 16):   # fewer, as many and more threads than blobs
        out = ctypes.create_string_buffer(32 * 5)
        L.c_kzg_blob_challenges(5, b"".join(BLOBS), b"".join(COMMS), threads, out)
        assert out.raw == single.raw, threads


def test_quotients_of_three_polynomials_at_three_points(L):
    """k_fr_eval_quotient_many's lanes: a random polynomial at a random point, the zero polynomial at
    0 and a polynomial with only its top coefficient at a root of unity, each in its own slot"""
    rnd = random.Random(0x51A7)
    top = [0] * N
    top[N - 1] = rnd.randrange(1, R)
    polys = [[rnd.randrange(R) for _ in range(N)], [0] * N, top]
    zs = [rnd.randrange(R), 0, K.ROOTS_BRP[5]]
    le = lambda vs: b"".join(int(v).to_bytes(32, "little") for v in vs)   # noqa: E731
    q = ctypes.create_string_buffer(bytes([0xAA]) * (32 * 3 * N), 32 * 3 * N)
    y = ctypes.create_string_buffer(32 * 3)
    L.c_fr_eval_quotient_many(3, N, le([v for p in polys for v in p]), le(zs), q, y)
    for k in range(3):
        exp_y, exp_q = S.synthetic_division(polys[k], zs[k])
        got_q = [int.from_bytes(q.raw[32 * (k * N + i): 32 * (k * N + i + 1)], "little") for i in range(N)]
        assert got_q == exp_q + [0], k
        assert int.from_bytes(y.raw[32 * k: 32 * k + 32], "little") == exp_y, k
    assert int.from_bytes(y.raw[64:96], "little") == top[N - 1] * pow(K.ROOTS_BRP[5], N - 1, R) % R


def _fold(L, offsets, k, bst, tst):
    nb = offsets[-1]
    b = np.asarray(bst + [OK], np.int32)
    t = np.asarray(tst, np.int32)
    return L.c_kzg_group_status(b.ctypes.data_as(I32), t.ctypes.data_as(I32), nb, offsets[k], offsets[k + 1])


def test_status_fold(L):
    """groups of 0, 1 and 3 blobs (offsets 0,0,1,4): every error kind at every position, and two
    errors in one group, where the lower index (then commitment, blob element, proof) wins"""
    offsets, nb, n = [0, 0, 1, 4], 4, 3
    clean_b, clean_t = [OK] * nb, [OK] * (3 * nb + n)
    for k in range(n):
        assert _fold(L, offsets, k, clean_b, clean_t) == OK
    for j in range(nb):
        k = 1 if j == 0 else 2
        for kind, code in (("c", NOT_IN_GROUP), ("c", BAD_ENCODING), ("b", BAD_SCALAR), ("p", NOT_IN_GROUP), ("p", BAD_ENCODING)):
            bst, tst = list(clean_b), list(clean_t)
            if kind == "c":
                tst[j] = code
            elif kind == "b":
                bst[j] = BAD_SCALAR
            else:
                tst[nb + j] = tst[2 * nb + j] = code    # the proof stands in two terms
            for g in range(n):
                assert _fold(L, offsets, g, bst, tst) == (code if g == k else OK), (j, kind, g)
    # two errors in the group of three (blobs 1, 2, 3)
    bst, tst = list(clean_b), list(clean_t)
    bst[3] = BAD_SCALAR
    tst[2 * nb + 2] = tst[nb + 2] = NOT_IN_GROUP          # blob 2's proof before blob 3's element
    assert _fold(L, offsets, 2, bst, tst) == NOT_IN_GROUP
    tst[2] = BAD_ENCODING                                  # blob 2's commitment before its proof
    assert _fold(L, offsets, 2, bst, tst) == BAD_ENCODING
    bst[1] = BAD_SCALAR                                    # blob 1's element before everything of blob 2
    assert _fold(L, offsets, 2, bst, tst) == BAD_SCALAR
    tst[1] = NOT_IN_GROUP                                  # blob 1's commitment before its element
    assert _fold(L, offsets, 2, bst, tst) == NOT_IN_GROUP
    assert _fold(L, offsets, 1, bst, tst) == OK and _fold(L, offsets, 0, bst, tst) == OK
    # a blob element error reads as LB_BAD_SCALAR whatever the kernel stored
    bst, tst = list(clean_b), list(clean_t)
    bst[0] = 5
    assert _fold(L, offsets, 1, bst, tst) == BAD_SCALAR


def test_offsets_validator(L):
    """the batched calls' offsets (lb_kzg_host.h kzg_offsets_ok): start at 0, never decrease, total
    within the cap; empty groups anywhere; a null pointer is refused, not read"""
    def ok(off, cap):
        a = np.asarray(off, np.uint32)
        return L.c_kzg_offsets_ok(len(off) - 1, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap)

    assert ok([0, 0, 1, 4], 4) == 1 and ok([0, 0, 1, 4], 1024) == 1
    assert ok([0, 0], 0) == 1 and ok([0, 3, 3, 3], 3) == 1       # empty groups, an empty call's total
    assert ok([0, 0, 1, 4], 3) == 0                              # total above the cap
    assert ok([1, 1, 4], 1024) == 0                              # does not start at 0
    assert ok([0, 2, 1, 4], 1024) == 0 and ok([0, 2, 4, 3], 1024) == 0   # decreases, in the middle and at the end
    assert ok([0, 0xFFFFFFFF], 1024) == 0 and ok([0, 0xFFFFFFFF], 0xFFFFFFFF) == 1
    assert L.c_kzg_offsets_ok(3, None, 1024) == 0


def test_item_status_fold_and_zero_fill(L):
    """the per-item fold of the compute calls (lb_kzg_host.h kzg_fold_status): the first list's code
    wins over the second's, a rejected item's outputs are zeroed at each output's own stride, its
    neighbours' bytes stay; one list and one output alone (null second list, null second output)"""
    first = np.asarray([OK, NOT_IN_GROUP, OK, BAD_ENCODING], np.int32)
    second = np.asarray([OK, BAD_SCALAR, BAD_SCALAR, OK], np.int32)
    st = np.full(4, -1, np.int32)
    a, b = ctypes.create_string_buffer(b"\xaa" * (4 * 48), 4 * 48), ctypes.create_string_buffer(b"\xbb" * (4 * 5), 4 * 5)
    L.c_kzg_fold_status(4, first.ctypes.data_as(I32), second.ctypes.data_as(I32), st.ctypes.data_as(I32), a, 48, b, 5)
    assert st.tolist() == [OK, NOT_IN_GROUP, BAD_SCALAR, BAD_ENCODING]
    assert a.raw == b"\xaa" * 48 + bytes(3 * 48) and b.raw == b"\xbb" * 5 + bytes(3 * 5)
    st = np.full(3, -1, np.int32)
    a = ctypes.create_string_buffer(b"\xaa" * (3 * 48), 3 * 48)
    one = np.asarray([OK, BAD_SCALAR, OK], np.int32)
    L.c_kzg_fold_status(3, one.ctypes.data_as(I32), None, st.ctypes.data_as(I32), a, 48, None, 0)
    assert st.tolist() == [OK, BAD_SCALAR, OK]
    assert a.raw == b"\xaa" * 48 + bytes(48) + b"\xaa" * 48


def test_low_degree_proof_through_the_python_pairing():
    """p(X) = 5 + 3 X + 0 X^2 + 2 X^3: commitment, challenge, value and proof by the oracle alone;
    the helper's batch equation (n = 1) accepts them and rejects y + 1"""
    g1, g2 = K.read_trusted_setup_bin(open(K.TRUSTED_SETUP_BIN, "rb").read())
    blob, c, z, y, proof = S.low_degree_proof(g1, [5, 3, 0, 2])
    assert S.evaluate_blob(blob, z) == y            # the barycentric route agrees with Horner
    assert z == K.compute_challenge(blob, c)
    assert S.batch_equation([c], [z], [y], [proof], g2) is True
    assert S.batch_equation([c], [z], [(y + 1) % R], [proof], g2) is False
    assert S.batch_equation([], [], [], [], g2) is True


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_blob_pieces_under_sanitizers(tmp_path):
    """tests/native/kzg_blob_check.cpp: the harness cases in a program of its own, built with
    -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "kzg_blob_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "harness"),
                    os.path.join(ROOT, "tests", "native", "kzg_blob_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kzg_blob_check: failures 0" in out.stdout
