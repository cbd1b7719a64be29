"""lb_block_sets_from_ssz on the GPU (signing_roots.block_signature_sets_ssz): the block signature sets of
SignedBeaconBlocks handed over as SSZ bytes.  The K3 devnet block from bytes equals the JSON walk and
verifies with the K3 keys; the smallest shapes at which the workgroup folds can go wrong give the oracle's
block root; a malformed block changes nothing for its neighbours; a dozen entries of the hostile corpus of
tests/test_ssz_sets_cpu.py give the statuses and rows of the CPU build of the same headers; both branches
of the sync rule, skip-proposer, every argument error; 32 blocks in one call make one stream
synchronisation (the engine's own count, lb_block_sets_syncs: the library has no other hook)."""
import copy
import ctypes

import numpy as np
import pytest

import ssz_codec as C
from conftest import load_json
from lodestar_amd import _native as N
from lodestar_amd import signing_roots as SR
from test_signing_roots import cpu_merkleize, k3_state
from test_ssz_sets_cpu import REAL_BLOCK, Setting, build, hostile_cases, run

pytestmark = pytest.mark.gpu
# kinds whose reference carries a byte position: attester slashing, attestation, sync aggregate, BLS change
POSITIONED = (2, 3, 6, 7)


@pytest.fixture(scope="module")
def k3():
    return load_json("k3_devnet.json")


def synthetic_state(k3, fork=3):
    """the K3 state's fork data with keys for any index: a validator's key is its index, a committee is
    0 .. 2047 (the operations blocks name validators and committees the devnet state does not have)"""
    import dataclasses
    return dataclasses.replace(k3_state(k3), pubkey=lambda i: i.to_bytes(4, "big"),
                               beacon_committee=lambda slot, index: list(range(2048)),
                               sync_committee=lambda: [i.to_bytes(4, "big") for i in range(512)],
                               fork_seq=lambda slot: fork)


def raw_call(engine, st, blocks, forks, state_slots, flags=0):
    """lb_block_sets_from_ssz itself -> (return code, [(status, rows)]) with rows as ssz_codec.expected_rows"""
    n = len(blocks)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(b) for b in blocks])
    ssz = np.frombuffer(b"".join(blocks) or b"\0", dtype=np.uint8)
    dom = np.frombuffer(st.dom * n, dtype=np.uint8)
    rows = n * 199
    status, n_sets = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint32)
    kind, roots = np.zeros(rows, dtype=np.uint32), np.zeros((rows, 32), dtype=np.uint8)
    sigs, ref = np.zeros((rows, 96), dtype=np.uint8), np.zeros((rows, 4), dtype=np.uint64)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    rc = engine.lib.lb_block_sets_from_ssz(
        engine.h, n, P(off, ctypes.c_uint32), P(ssz, ctypes.c_uint8), P(np.asarray(forks, dtype=np.uint32), ctypes.c_uint32),
        P(dom, ctypes.c_uint8), P(np.full(n, st.fork_epoch, dtype=np.uint64), ctypes.c_uint64),
        P(np.asarray(state_slots, dtype=np.uint64), ctypes.c_uint64), flags, P(status, ctypes.c_int32),
        P(n_sets, ctypes.c_uint32), P(kind, ctypes.c_uint32), P(roots, ctypes.c_uint8), P(sigs, ctypes.c_uint8),
        P(ref, ctypes.c_uint64))
    out = []
    for b in range(n):
        r = range(199 * b, 199 * b + int(n_sets[b]))
        base = int(off[b])  # positions are in the call's buffer: make them the block's, as the CPU program's are
        out.append((int(status[b]), [(int(kind[i]), roots[i].tobytes(), sigs[i].tobytes(),
                                      tuple(int(x) - (base if j == 2 and int(kind[i]) in POSITIONED else 0)
                                            for j, x in enumerate(ref[i]))) for i in r]))
    return rc, out


def test_k3_from_bytes_equals_the_json_walk_and_verifies(engine, k3):
    from lodestar_amd.engine import SetInput
    pk96 = {}

    def pub(b48):
        if b48 not in pk96:
            out, st = engine.g1_decompress([b48])
            assert st == [0]
            pk96[b48] = out[0]
        return pk96[b48]
    state = k3_state(k3, pub)
    want = SR.resolve(SR.block_signature_sets(k3["signed_block"], state), cpu_merkleize)
    raw = C.encode_signed_block(k3["signed_block"], 3)
    got, = SR.block_signature_sets_ssz(engine, [raw], [state])
    assert [s.name for s in got] == ["randao", "attestation", "proposer", "sync_aggregate"]
    assert got == want
    gold = {g["name"].split("_slot")[0]: g["signing_root"] for g in k3["sets"]}
    assert [s.signing_root.hex() for s in got] == [gold[s.name] for s in got]
    jobs = [[SetInput(s.pubkeys, s.signing_root, s.signature)] for s in got]
    assert engine.verify_jobs(jobs) == [1, 1, 1, 1]
    assert engine.verify_jobs([[j[0] for j in jobs]]) == [1]
    sync = [s for s in got if s.name == "sync_aggregate"][0]
    assert engine.verify_jobs([[SetInput(sync.pubkeys[1:], sync.signing_root, sync.signature)]]) == [0]
    # the operations block and every fork through the Python surface, against the JSON walk
    for blk, fork in [(C.every_operation_block(k3), 3)] + [(C.fork_block(k3, f), f) for f in range(3)]:
        st = synthetic_state(k3, fork)
        want = SR.resolve(SR.block_signature_sets(blk, st), cpu_merkleize)
        got, = SR.block_signature_sets_ssz(engine, [C.encode_signed_block(blk, fork)], [st])
        assert got == want, fork


def boundary_blocks(k3):
    """the smallest shapes at which a parallel fold can go wrong, over the K3 capella block"""
    slot = int(k3["signed_block"]["message"]["slot"])
    out = []

    def variant(**kw):
        blk = copy.deepcopy(k3["signed_block"])
        b = blk["message"]["body"]
        for key in ("transactions", "extra_data"):
            if key in kw:
                b["execution_payload"][key] = kw[key]
        for key in ("attestations", "attester_slashings"):
            if key in kw:
                b[key] = kw[key]
        out.append(blk)
    variant(transactions=[])
    variant(transactions=[C.tx(0)], extra_data="0x")
    variant(transactions=[C.tx(32)], extra_data="0x" + "e1" * 32)
    variant(transactions=[C.tx(33)])
    variant(transactions=[C.tx(32 * 65)])
    variant(transactions=[C.tx(32 * 65, 2), C.tx(0), C.tx(33, 4), C.tx(32, 5), C.tx(1, 6), C.tx(64, 7), C.tx(63, 8)])
    variant(attester_slashings=[{"attestation_1": C.indexed([], slot - 3, "d1"), "attestation_2": C.indexed([7], slot - 3, "d2")},
                                {"attestation_1": C.indexed([1, 2, 3, 4], 40, "d3"),
                                 "attestation_2": C.indexed([1, 2, 3, 4, 5], 40, "d4")}])
    variant(attestations=[C.attestation(slot - 1, i, n, "%02x" % (0x60 + i)) for i, n in enumerate((0, 8, 255, 256, 257, 2048))])
    variant(attestations=[])
    variant(attestations=[C.attestation(slot - 1 - i % 3, i % 64, 1 + (37 * i) % 300, "%02x" % i) for i in range(128)])
    return out


def test_boundary_shapes_give_the_oracle_block_root(engine, k3):
    st = Setting(k3)
    slot = int(k3["signed_block"]["message"]["slot"])
    blocks = boundary_blocks(k3)
    raws = [C.encode_signed_block(b, 3) for b in blocks]
    rc, got = raw_call(engine, st, raws, [3] * len(raws), [slot] * len(raws))
    assert rc == 0
    for i, (blk, raw, (status, rows)) in enumerate(zip(blocks, raws, got)):
        want_status, want_rows, want_root = st.expected(blk, raw, 3, slot)
        assert status == 0 and want_status == "ok", i
        prop = [r for r in rows if r[0] == C.KINDS.index("proposer")]
        assert len(prop) == 1 and prop[0][1] == [r for r in want_rows if r[0] == 5][0][1], i  # H(block root, domain)
        assert rows == want_rows, i


def test_real_bellatrix_block(engine, k3):
    """139 405 bytes, about 135 KB of transactions: block root and attestation roots"""
    raw = open(REAL_BLOCK, "rb").read()
    blk = C.decode_signed_block(raw, 2)
    st = Setting(k3)
    rc, ((status, rows),) = raw_call(engine, st, [raw], [2], [13249])
    want_status, want_rows, _ = st.expected(blk, raw, 2, 13249)
    assert (rc, status) == (0, 0) and rows == want_rows


def test_isolation_hostile_statuses_sync_rule_and_skip_proposer(engine, k3, tmp_path):
    st = Setting(k3)
    slot = int(k3["signed_block"]["message"]["slot"])
    good = C.encode_signed_block(C.every_operation_block(k3), 3)
    k3raw = C.encode_signed_block(k3["signed_block"], 3)
    alone = raw_call(engine, st, [good], [3], [slot])[1][0]
    assert alone[0] == 0
    # a dozen of the corpus that ran under the sanitizers on the CPU: prefixes, and offsets of each replacement
    corpus = {label: (fork, data) for label, fork, data in hostile_cases(k3)}
    labels = ["p0_cut0", "ops_cut%d" % (len(good) - 344), "p0_cut403", "ops_cut%d" % (len(good) - 1), "ops_cut%d" % (len(good) - 172),
              "ops_cut5000"] + [next(x for x in corpus if x.startswith("ops_off") and x.endswith(suffix) and int(x[7:].split("_")[0]) > lo)
                                for suffix, lo in (("_zero", 0), ("_minus1", 400), ("_plus1", 600), ("_end", 700),
                                                   ("_end1", 300), ("_ones", 900))]
    assert len(set(labels)) == 12
    picked = [corpus[x] for x in labels]
    cpu = run(build(tmp_path, "ssz_walk_check", []), tmp_path, [st.case(d, f, slot) for f, d in picked])
    # one call: good, hostile..., good -- and a malformed block between two good ones among them
    blocks = [good] + [d for _, d in picked] + [k3raw]
    rc, got = raw_call(engine, st, blocks, [3] + [f for f, _ in picked] + [3], [slot] * len(blocks))
    assert rc == 0
    assert [(g[0], g[1]) for g in got[1:-1]] == [(c[0], c[2]) for c in cpu]
    assert any(c[0] == 1 for c in cpu) and any(c[0] == 0 for c in cpu)
    assert got[0] == alone and got[-1] == raw_call(engine, st, [k3raw], [3], [slot])[1][0]
    rc, three = raw_call(engine, st, [good, good[:5000], k3raw], [3, 3, 3], [slot] * 3)
    assert rc == 0 and three[1] == (1, []) and three[0] == alone and three[2] == got[-1]
    # the sync rule: no participant and infinity -> no set; anything else -> LB_VERIFY_FAIL, "Empty sync
    # committee signature is not infinity"
    sync_blocks = []
    for sig in ("0xc0" + "00" * 95, k3["signed_block"]["message"]["body"]["sync_aggregate"]["sync_committee_signature"]):
        blk = copy.deepcopy(k3["signed_block"])
        blk["message"]["body"]["sync_aggregate"] = {"sync_committee_bits": "0x" + "00" * 64, "sync_committee_signature": sig}
        sync_blocks.append(blk)
    res = SR.block_signature_sets_ssz(engine, [C.encode_signed_block(b, 3) for b in sync_blocks] + [good[:300]],
                                      [k3_state(k3)] * 3)
    assert [s.name for s in res[0]] == ["randao", "attestation", "proposer"]
    assert res[0] == SR.resolve(SR.block_signature_sets(sync_blocks[0], k3_state(k3)), cpu_merkleize)
    assert isinstance(res[1], ValueError) and str(res[1]) == "Empty sync committee signature is not infinity"
    assert isinstance(res[2], ValueError) and "BAD_ENCODING" in str(res[2]).upper().replace(" ", "_")
    # skip proposer
    rc, skipped = raw_call(engine, st, [good], [3], [slot], flags=1)
    assert rc == 0 and skipped[0] == (0, [r for r in alone[1] if r[0] != C.KINDS.index("proposer")])
    py, = SR.block_signature_sets_ssz(engine, [good], [synthetic_state(k3)], skip_proposer_signature=True)
    assert py == SR.resolve(SR.block_signature_sets(C.every_operation_block(k3), synthetic_state(k3), True), cpu_merkleize)


def test_argument_errors(engine, k3):
    st = Setting(k3)
    raw = C.encode_signed_block(k3["signed_block"], 3)
    lib, h = engine.lib, engine.h
    n = 2
    off = np.asarray([0, len(raw), 2 * len(raw)], dtype=np.uint32)
    ssz = np.frombuffer(raw * 2, dtype=np.uint8)
    arrays = dict(off=off, ssz=ssz, forks=np.full(n, 3, dtype=np.uint32), dom=np.frombuffer(st.dom * n, dtype=np.uint8),
                  fe=np.full(n, st.fork_epoch, dtype=np.uint64), ss=np.zeros(n, dtype=np.uint64),
                  status=np.zeros(n, dtype=np.int32), n_sets=np.zeros(n, dtype=np.uint32),
                  kind=np.zeros(199 * n, dtype=np.uint32), roots=np.zeros(199 * n * 32, dtype=np.uint8),
                  sigs=np.zeros(199 * n * 96, dtype=np.uint8), ref=np.zeros(199 * n * 4, dtype=np.uint64))
    types = dict(off=ctypes.c_uint32, ssz=ctypes.c_uint8, forks=ctypes.c_uint32, dom=ctypes.c_uint8, fe=ctypes.c_uint64,
                 ss=ctypes.c_uint64, status=ctypes.c_int32, n_sets=ctypes.c_uint32, kind=ctypes.c_uint32,
                 roots=ctypes.c_uint8, sigs=ctypes.c_uint8, ref=ctypes.c_uint64)

    def call(n_blocks=n, engine_h=h, **over):
        a = {k: over.get(k, v) for k, v in arrays.items()}
        p = {k: (None if a[k] is None else a[k].ctypes.data_as(ctypes.POINTER(types[k]))) for k in a}
        return lib.lb_block_sets_from_ssz(engine_h, n_blocks, p["off"], p["ssz"], p["forks"], p["dom"], p["fe"], p["ss"], 0,
                                          p["status"], p["n_sets"], p["kind"], p["roots"], p["sigs"], p["ref"])
    before = lib.lb_block_sets_syncs(h)
    assert call() == N.LB_OK and arrays["status"].tolist() == [0, 0] and arrays["n_sets"].tolist() == [4, 4]
    assert lib.lb_block_sets_syncs(h) == before + 1
    for name in arrays:  # every pointer is needed
        assert call(**{name: None}) == N.LB_ERR_ARGUMENT, name
    assert call(engine_h=None) == N.LB_ERR_ARGUMENT
    assert call(off=np.asarray([1, len(raw), 2 * len(raw)], dtype=np.uint32)) == N.LB_ERR_ARGUMENT
    assert call(off=np.asarray([0, len(raw), len(raw) - 1], dtype=np.uint32)) == N.LB_ERR_ARGUMENT
    assert call(forks=np.asarray([3, 4], dtype=np.uint32)) == N.LB_ERR_ARGUMENT  # deneb and later
    assert call(n_blocks=65, off=np.zeros(66, dtype=np.uint32)) == N.LB_ERR_ARGUMENT
    assert call(off=np.asarray([0, len(raw), (64 << 20) + 1], dtype=np.uint32)) == N.LB_ERR_ARGUMENT
    assert lib.lb_block_sets_syncs(h) == before + 1  # nothing was launched
    assert call(n_blocks=0, off=None, ssz=None, status=None) == N.LB_OK  # returns at once


def test_32_blocks_one_synchronisation(engine, k3):
    """a 32-block segment in one call: one stream synchronisation, and every block's sets as alone"""
    st = Setting(k3)
    slot = int(k3["signed_block"]["message"]["slot"])
    pool = [C.encode_signed_block(b, 3) for b in boundary_blocks(k3)[4:8]] + [C.encode_signed_block(k3["signed_block"], 3)]
    blocks = [pool[i % len(pool)] for i in range(32)]
    alone = [raw_call(engine, st, [b], [3], [slot])[1][0] for b in pool]
    before = engine.lib.lb_block_sets_syncs(engine.h)
    rc, got = raw_call(engine, st, blocks, [3] * 32, [slot] * 32)
    assert rc == 0 and engine.lib.lb_block_sets_syncs(engine.h) == before + 1
    assert got == [alone[i % len(pool)] for i in range(32)]
