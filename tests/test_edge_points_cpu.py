"""tests/golden/edge_points.json (make_edge_points.py) on the CPU: the generator reproduces the
committed file byte for byte, and the device's point decoders compiled for x86 (tests/harness/
lb_harness.cpp: g2_decompress96, g1_decompress48, g1_deserialize96, the compressors, and the
[r]P == O key validation by jac_mul_u256) give the oracle's status and point for every record.
tests/native/edge_points_check.cpp does the same in a program of its own under the address and
undefined-behaviour sanitizers.  All comparisons are exact.  tests/test_edge_points_gpu.py runs the same records through the
kernels, whose square-root exponentiations do not exist on x86."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT, load_json
from oracle import bls_oracle as o

STATUS_NAME = {0: "ok", 1: "BLST_BAD_ENCODING", 2: "BLST_POINT_NOT_ON_CURVE"}


@pytest.fixture(scope="module")
def L():
    from lodestar_amd.build import build_harness
    return ctypes.CDLL(build_harness(verbose=False))


def records(kind):
    return [r for r in load_json("edge_points.json")["records"] if r["kind"] == kind]


def test_generator_reproduces_the_fixture(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_edge_points
    finally:
        sys.path.pop(0)
    out = tmp_path / "edge_points.json"
    make_edge_points.main(str(out))
    with open(os.path.join(ROOT, "tests", "golden", "edge_points.json"), "rb") as f:
        assert out.read_bytes() == f.read()


def test_fixture_holds_what_the_gpu_tests_rely_on():
    recs = load_json("edge_points.json")["records"]
    for kind in ("g2c96", "g1c48", "g1u96"):
        mine = [r for r in recs if r["kind"] == kind]
        assert {r["status"] for r in mine} == {"ok", "inf", "BLST_BAD_ENCODING", "BLST_POINT_NOT_ON_CURVE"}
        assert "BLST_POINT_NOT_IN_GROUP" in {r["status_validated"] for r in mine}
    tags = {t for r in recs if r["kind"] == "g2c96" for t in r["tags"]}
    assert {"y_c1_zero", "y_c0_zero", "d1_zero", "rhs_c0_zero"} <= tags
    for kind in ("g1c48", "g1u96"):
        tags = {t for r in recs if r["kind"] == kind for t in r["tags"]}
        assert {"key", "neg_key", "order3", "order11", "mixed", "infinity"} <= tags
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "edge_points.json")) < 100_000


def test_oracle_rejects_flag_20_on_uncompressed_keys():
    """blst takes only 000 in the top three bits as uncompressed; the device always did"""
    (r,) = [r for r in records("g1u96") if "flag_20" in r["tags"]]
    b = bytes.fromhex(r["hex"])
    assert b[0] & 0xE0 == 0x20 and r["status"] == "BLST_BAD_ENCODING"
    with pytest.raises(o.BlsError, match="BLST_BAD_ENCODING"):
        o.g1_deserialize(b)
    assert o.g1_deserialize(bytes([b[0] & 0x1F]) + b[1:]) is not None


def test_g2_records_through_the_x86_decoder(L):
    inf = ctypes.c_int()
    o192, o96 = ctypes.create_string_buffer(192), ctypes.create_string_buffer(96)
    seen = 0
    for r in records("g2c96"):
        b = bytes.fromhex(r["hex"])
        st = L.h_g2_decompress(b, o192, ctypes.byref(inf))
        assert ("inf" if st == 0 and inf.value else STATUS_NAME[st]) == r["status"], r["name"]
        if r["status"] != "ok":
            continue
        raw = o192.raw                                   # harness order: x.c0 x.c1 y.c0 y.c1
        assert (raw[48:96] + raw[:48] + raw[144:] + raw[96:144]).hex() == r["point"], r["name"]
        L.h_g2_compress(raw, o96)
        assert o96.raw == b, r["name"]
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("kind", ["g1c48", "g1u96"])
def test_g1_records_through_the_x86_decoders(L, kind):
    inf = ctypes.c_int()
    o96, o48 = ctypes.create_string_buffer(96), ctypes.create_string_buffer(48)
    decode = L.h_g1_decompress if kind == "g1c48" else L.h_g1_deserialize
    validated = set()
    for r in records(kind):
        b = bytes.fromhex(r["hex"])
        st = decode(b, o96, ctypes.byref(inf))
        assert ("inf" if st == 0 and inf.value else STATUS_NAME[st]) == r["status"], r["name"]
        if r["status"] == "inf":
            assert r["status_validated"] == "BLST_PK_IS_INFINITY"
        if r["status"] != "ok":
            continue
        assert o96.raw.hex() == r["point"], r["name"]
        if kind == "g1c48":
            L.h_g1_compress(o96.raw, o48)
            assert o48.raw == b, r["name"]
        else:
            assert o96.raw == b, r["name"]                # the uncompressed form is the point itself
        # keyValidate: [r]P == O, the kernels' jac_mul_u256 form
        in_group = bool(L.h_g1_in_subgroup_r(o96.raw))
        assert ("ok" if in_group else "BLST_POINT_NOT_IN_GROUP") == r["status_validated"], r["name"]
        validated.add(in_group)
    assert validated == {True, False}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_decoders_and_key_validation_under_sanitizers(tmp_path):
    """tests/native/edge_points_check.cpp: every record decoded from a heap block of exactly its size,
    validated and re-encoded in a program of its own, built with -fsanitize=address,undefined"""
    recs = load_json("edge_points.json")["records"]
    inp = tmp_path / "records.txt"
    inp.write_text("".join(f"{r['kind']} {r['hex']}\n" for r in recs))
    exe = tmp_path / "edge_points_check"
    subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "edge_points_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == f"edge_points_check: records {len(recs)}"
    for r, line in zip(recs, lines):
        st, inf, in_group, again = line.split()
        assert ("inf" if st == "0" and inf == "1" else STATUS_NAME[int(st)]) == r["status"], r["name"]
        if r["status"] == "ok":
            assert again == r["hex"], r["name"]
            if r["kind"] != "g2c96":
                assert ("ok" if in_group == "1" else "BLST_POINT_NOT_IN_GROUP") == r["status_validated"], r["name"]
        else:
            assert in_group == "-", r["name"]
