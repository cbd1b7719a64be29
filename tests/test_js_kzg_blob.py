"""tests/js/test_kzg_blob.js: the per-blob (Deneb) c-kzg names of lodestar_amd/js/kzg.js.  Without a
GPU: argument validation and the two transcripts against Python.  On the GPU: the JS names give the
bytes and verdicts of the Python surface for groups of 0, 1, 2, 0 and 3 blobs."""
import json
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_deneb_spec as S  # noqa: E402

from lodestar_amd import kzg as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_kzg_blob.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")
R = K.BLS_MODULUS


def _run(*args):
    if NODE is None:
        pytest.skip("node not installed")
    if not os.path.exists(ADDON):
        from lodestar_amd.build import build_napi
        build_napi(verbose=False)
    r = subprocess.run([NODE, SCRIPT, *args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"js kzg blob {args[0]} ok", r.stdout
    return json.loads(lines[-2])


def _sequential_blob(off):
    return b"".join(((i + off) & 0xFFFFFFFF).to_bytes(4, "big") + bytes(28) for i in range(4096))


def test_js_transcripts_match_python():
    got = _run("cpu")
    blob, c, p = _sequential_blob(3), b"\x11" * 48, b"\x22" * 48
    z, z0 = K.compute_challenge(blob, c), K.compute_challenge(bytes(K.BYTES_PER_BLOB), c)
    assert (int(got["z"]), int(got["z0"])) == (z, z0) == (S.compute_challenge(blob, c), S.compute_challenge(bytes(K.BYTES_PER_BLOB), c))
    zs, ys = [z, 0, R - 1], [5, R - 1, 0]
    exp = [K.compute_batch_r([c] * n, zs[:n], ys[:n], [p] * n) for n in (0, 1, 3)]
    assert [int(v) for v in got["r"]] == exp == [S.compute_batch_r([c] * n, zs[:n], ys[:n], [p] * n) for n in (0, 1, 3)]


@pytest.mark.gpu
def test_js_names_match_the_python_surface(engine, tmp_path):
    from test_kzg_blob import BLOBS, SIZES
    path = tmp_path / "blobs.bin"
    path.write_bytes(b"".join(BLOBS))
    got = _run("gpu", str(path))
    dev = K.Kzg(engine, field="device")
    comms = dev._device_commitments(BLOBS)
    proofs = [dev.compute_blob_kzg_proof(b, c) for b, c in zip(BLOBS, comms)]
    assert got["commitments"] == [c.hex() for c in comms]
    assert got["proofs"] == [p.hex() for p in proofs]

    def many(blobs, cs, ps):
        groups, at = [], 0
        for n in SIZES:
            groups.append((blobs[at: at + n], cs[at: at + n], ps[at: at + n]))
            at += n
        return [f"Error: {str(v).split(': ', 1)[1]}" if isinstance(v, K.KzgError) else v
                for v in dev.verify_blob_kzg_proof_batch_many(groups)]

    def sub(lst, j, v):
        return lst[:j] + [v] + lst[j + 1:]

    elem_r = BLOBS[2][:-32] + R.to_bytes(32, "big")
    flagless = bytes([comms[4][0] & 0x7F]) + comms[4][1:]
    assert got["valid"] == many(BLOBS, comms, proofs) == [True] * 5
    assert got["tampered"] == many(BLOBS, comms, sub(proofs, 5, proofs[1])) == [True, True, True, True, False]
    assert got["swapped"] == many(BLOBS, comms, sub(sub(proofs, 1, proofs[2]), 2, proofs[1])) == [True, True, False, True, True]
    assert got["elemR"] == many(sub(BLOBS, 2, elem_r), comms, proofs)
    assert got["elemR"][2] == "Error: BLST_BAD_SCALAR"
    assert got["flagless"] == many(BLOBS, sub(comms, 4, flagless), proofs)
    assert got["flagless"][4].startswith("Error: ") and got["flagless"][:4] == [True] * 4
    assert got["single"] == [dev.verify_blob_kzg_proof(BLOBS[1], comms[1], proofs[1]),
                             dev.verify_blob_kzg_proof(BLOBS[1], comms[1], proofs[2])] == [True, False]
    assert got["batch"] == [True, True, False]
    z = bytes(5) + b"\x12" + bytes(25) + b"\x05"
    proof, y = dev.compute_kzg_proof_bytes(BLOBS[2], z)
    assert got["point"] == [proof.hex(), y.hex()]
    assert got["pointOk"] == [True, False]
