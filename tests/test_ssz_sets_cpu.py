"""lb_block_sets_from_ssz on the CPU: csrc/lb_ssz_walk.h and the root functions of csrc/lb_ssz_sets.h
built with g++ into tests/native/ssz_walk_check.cpp, on one thread.

Parity: roots, kinds, signatures and key references equal block_signature_sets + oracle/ssz.py on the
same JSON (tests/ssz_codec.py encodes it) for the K3 capella block, a block carrying every operation
type and one block per fork.  Hostile corpus: the smallest phase0 block and the every-operation
capella block cut at every prefix length and with every offset word replaced by 0, its value - 1 and
+ 1, its container's end, the end + 1 and 0xFFFFFFFF; each result is LB_BAD_ENCODING or a parse the
independent decoder of tests/ssz_codec.py accepts with equal rows.  The same corpus runs through a
second build with -fsanitize=address,undefined, each input in a heap buffer of its exact length.
The reference's real bellatrix block (tests/golden/goerli_shadow_fork_block_13249.ssz, 139 405 bytes,
slot 13249): block root and attestation roots against the decoder + oracle/ssz.py.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

import ssz_codec as C
from conftest import ROOT, load_json

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
SRC = os.path.join(ROOT, "tests", "native", "ssz_walk_check.cpp")
REAL_BLOCK = os.path.join(ROOT, "tests", "golden", "goerli_shadow_fork_block_13249.ssz")


def build(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-DLB_KGROUP=99", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "lodestar_amd", "csrc"), SRC, "-o", exe], check=True)
    return exe


def run(exe, tmp, cases, name="cases.bin"):
    path = os.path.join(str(tmp), name)
    C.write_cases(path, cases)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
    return C.parse_output(out.stdout)


class Setting:
    """the K3 devnet state's fork data: what the call takes beside the bytes"""

    def __init__(self, k3):
        self.gvr = bytes.fromhex(k3["genesis_validators_root"])
        self.prev_v = bytes.fromhex(k3["fork"]["previous_version"])
        self.cur_v = bytes.fromhex(k3["fork"]["current_version"])
        self.fork_epoch = int(k3["fork"]["epoch"])
        self.dom = C.domains32(self.gvr, self.prev_v, self.cur_v)

    def case(self, raw, fork, state_slot, skip=False):
        return (fork, 1 if skip else 0, self.fork_epoch, state_slot, self.dom, raw)

    def expected(self, blk, raw, fork, state_slot, skip=False):
        return C.expected_rows(blk, raw, fork, self.gvr, self.prev_v, self.cur_v, self.fork_epoch, state_slot, skip)


@pytest.fixture(scope="module")
def k3():
    return load_json("k3_devnet.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ssz_walk")


@pytest.fixture(scope="module")
def exe(tmp):
    return build(tmp, "ssz_walk_check", [])


@pytest.fixture(scope="module")
def exe_san(tmp):
    return build(tmp, "ssz_walk_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def parity_blocks(k3):
    """(name, JSON, fork, state slot, skip proposer)"""
    slot = int(k3["signed_block"]["message"]["slot"])
    out = [("k3", k3["signed_block"], 3, slot, False), ("every_operation", C.every_operation_block(k3), 3, slot, False),
           ("every_operation_skip", C.every_operation_block(k3), 3, slot, True),
           # a state one fork epoch back: the BLS change takes the previous version
           ("every_operation_old_state", C.every_operation_block(k3), 3, 0, False)]
    out += [("fork%d" % f, C.fork_block(k3, f), f, slot, False) for f in range(4)]
    ops = C.every_operation_block(k3)
    for f in range(3):
        b = C.fork_block({"signed_block": ops}, f)
        out.append(("every_operation_fork%d" % f, b, f, slot, False))
    return out


def test_codec_round_trip(k3):
    """the encoder and the decoder are each other's inverse on every parity block, and the K3 block's
    encoding has the body root the reference's post-state pins"""
    for name, blk, fork, _, _ in parity_blocks(k3):
        raw = C.encode_signed_block(blk, fork)
        assert C.decode_signed_block(raw, fork) == C.canonical(blk), name
    raw = C.encode_signed_block(C.smallest_phase0_block(), 0)
    assert len(raw) == 100 + 84 + 220 and C.decode_signed_block(raw, 0) == C.smallest_phase0_block()


def test_parity(k3, exe, tmp):
    st = Setting(k3)
    blocks = parity_blocks(k3)
    raws = [C.encode_signed_block(blk, fork) for _, blk, fork, _, _ in blocks]
    got = run(exe, tmp, [st.case(raw, fork, ss, skip) for raw, (_, _, fork, ss, skip) in zip(raws, blocks)], "parity.bin")
    for (name, blk, fork, ss, skip), raw, (status, root, rows) in zip(blocks, raws, got):
        want_status, want_rows, want_root = st.expected(blk, raw, fork, ss, skip)
        assert status == 0 and want_status == "ok", name
        assert root == want_root, name
        assert [r[0] for r in rows] == [r[0] for r in want_rows], name
        assert rows == want_rows, name
    # the K3 block's golden roots (tests/golden/make_k3.py), and every kind present in the operations block
    gold = {g["name"].split("_slot")[0]: g for g in k3["sets"]}
    assert got[0][1].hex() == k3["block_root"]
    assert [(C.KINDS[r[0]], r[1].hex(), r[2].hex()) for r in got[0][2]] == \
        [(n, gold[n]["signing_root"], gold[n]["signature"]) for n in ("randao", "attestation", "proposer", "sync_aggregate")]
    assert sorted({r[0] for r in got[1][2]}) == list(range(8))
    assert C.KINDS.index("proposer") not in {r[0] for r in got[2][2]}
    assert got[3][2][-1][1] != got[1][2][-1][1]  # the BLS change under the other fork version


def test_sync_rule(k3, exe, tmp):
    """no participant: no set with the signature at infinity, LB_VERIFY_FAIL with any other"""
    import copy
    st = Setting(k3)
    slot = int(k3["signed_block"]["message"]["slot"])
    cases, blocks = [], []
    for sig in ("0xc0" + "00" * 95, k3["signed_block"]["message"]["body"]["sync_aggregate"]["sync_committee_signature"],
                "0xc0" + "00" * 94 + "01"):
        blk = copy.deepcopy(k3["signed_block"])
        blk["message"]["body"]["sync_aggregate"] = {"sync_committee_bits": "0x" + "00" * 64, "sync_committee_signature": sig}
        blocks.append(blk)
        cases.append(st.case(C.encode_signed_block(blk, 3), 3, slot))
    got = run(exe, tmp, cases, "sync.bin")
    assert [g[0] for g in got] == [0, 5, 5]
    want = st.expected(blocks[0], cases[0][5], 3, slot)
    assert want[0] == "ok" and got[0][2] == want[1] and C.KINDS.index("sync_aggregate") not in {r[0] for r in want[1]}
    assert st.expected(blocks[1], cases[1][5], 3, slot)[0] == "verify_fail" and got[1][2] == []


def hostile_cases(k3):
    """[(label, fork, bytes)] of the whole hostile corpus"""
    out = []
    for tag, blk, fork in (("p0", C.smallest_phase0_block(), 0), ("ops", C.every_operation_block(k3), 3)):
        raw = C.encode_signed_block(blk, fork)
        out += [(tag + "_" + label, fork, data) for label, data in C.hostile_corpus(raw, fork)]
    return out


def check_hostile(k3, exe, tmp, name):
    st = Setting(k3)
    slot = int(k3["signed_block"]["message"]["slot"])
    corpus = hostile_cases(k3)
    got = run(exe, tmp, [st.case(data, fork, slot) for _, fork, data in corpus], name)
    assert len(got) == len(corpus) > 5000
    accepted = 0
    for (label, fork, data), (status, root, rows) in zip(corpus, got):
        if status == 1:
            continue
        accepted += 1
        blk = C.decode_signed_block(data, fork)  # raises if the independent decoder rejects it
        want_status, want_rows, want_root = st.expected(blk, data, fork, slot)
        assert (status, rows) == ({"ok": 0, "verify_fail": 5}[want_status], want_rows), label
        if status == 0:
            assert root == want_root, label
    # and the other way round: what the decoder accepts, the walk accepts (it is no stricter than SSZ)
    for (label, fork, data), (status, _, _) in zip(corpus, got):
        if status == 1 and not label.split("_")[1].startswith("cut"):
            with pytest.raises(ValueError):
                C.decode_signed_block(data, fork)
    return accepted, len(corpus)


def test_hostile_corpus(k3, exe, tmp):
    accepted, n = check_hostile(k3, exe, tmp, "hostile.bin")
    assert 0 < accepted < n // 4


def test_hostile_corpus_under_the_sanitizers(k3, exe_san, tmp):
    """the same corpus and the parity blocks through the address + undefined-behaviour build: every input
    sits in a heap buffer of its exact length, so a byte read outside [start, end) ends the run"""
    check_hostile(k3, exe_san, tmp, "hostile_san.bin")
    st = Setting(k3)
    run(exe_san, tmp, [st.case(C.encode_signed_block(blk, fork), fork, ss, skip)
                       for _, blk, fork, ss, skip in parity_blocks(k3)], "parity_san.bin")


def test_real_bellatrix_block(k3, exe, tmp):
    """packages/reqresp/test/fixtures/goerliShadowForkBlock.13249/serialized.ssz of the reference"""
    import oracle.ssz as S
    raw = open(REAL_BLOCK, "rb").read()
    assert len(raw) == 139405
    blk = C.decode_signed_block(raw, 2)
    assert blk["message"]["slot"] == "13249"
    assert C.encode_signed_block(blk, 2) == raw
    st = Setting(k3)
    (status, root, rows), = run(exe, tmp, [st.case(raw, 2, 13249)], "real.bin")
    want_status, want_rows, want_root = st.expected(blk, raw, 2, 13249)
    assert status == 0 and root == want_root == S.beacon_block(blk["message"], 2)
    assert rows == want_rows
    atts = blk["message"]["body"]["attestations"]
    assert len([r for r in rows if r[0] == 3]) == len(atts)
    assert sum(len(t) // 2 - 1 for t in blk["message"]["body"]["execution_payload"]["transactions"]) > 130000
