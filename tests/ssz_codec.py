"""Test-side SSZ codec for SignedBeaconBlock, phase0 .. capella (mainnet preset): an encoder from
the beacon API's JSON to SSZ bytes, which makes the inputs of lb_block_sets_from_ssz, and a strict
decoder back to JSON, written from the SSZ specification as a table of types and one generic
routine.  It shares nothing with csrc/lb_ssz_walk.h, so a parse the walk accepts can be checked
against it: the decoder accepts it too, and block_signature_sets + oracle/ssz.py on what it decoded
give the walk's rows (expected_rows).  Also the hostile corpus (truncations and offset
replacements) and the block builders the CPU and GPU tests share.  Test infrastructure only.
"""
import copy
import struct

# ------------------------------------------------------------------ types
U64, U256 = ("u64",), ("u256",)


def B(n):
    return ("bytes", n)


def C(*fields):
    return ("container", fields)


def L(elem, limit):
    return ("list", elem, limit)


BYTELIST = lambda limit: ("bytelist", limit)  # noqa: E731
BITLIST = lambda limit: ("bitlist", limit)  # noqa: E731

CHECKPOINT = C(("epoch", U64), ("root", B(32)))
ATT_DATA = C(("slot", U64), ("index", U64), ("beacon_block_root", B(32)), ("source", CHECKPOINT), ("target", CHECKPOINT))
ATTESTATION = C(("aggregation_bits", BITLIST(2048)), ("data", ATT_DATA), ("signature", B(96)))
INDEXED = C(("attesting_indices", L(U64, 2048)), ("data", ATT_DATA), ("signature", B(96)))
HEADER = C(("slot", U64), ("proposer_index", U64), ("parent_root", B(32)), ("state_root", B(32)), ("body_root", B(32)))
SIGNED_HEADER = C(("message", HEADER), ("signature", B(96)))
PROPOSER_SLASHING = C(("signed_header_1", SIGNED_HEADER), ("signed_header_2", SIGNED_HEADER))
ATTESTER_SLASHING = C(("attestation_1", INDEXED), ("attestation_2", INDEXED))
DEPOSIT = C(("proof", ("vector", B(32), 33)),
            ("data", C(("pubkey", B(48)), ("withdrawal_credentials", B(32)), ("amount", U64), ("signature", B(96)))))
SIGNED_EXIT = C(("message", C(("epoch", U64), ("validator_index", U64))), ("signature", B(96)))
SYNC_AGGREGATE = C(("sync_committee_bits", B(64)), ("sync_committee_signature", B(96)))
WITHDRAWAL = C(("index", U64), ("validator_index", U64), ("address", B(20)), ("amount", U64))
SIGNED_BLS_CHANGE = C(("message", C(("validator_index", U64), ("from_bls_pubkey", B(48)),
                                    ("to_execution_address", B(20)))), ("signature", B(96)))
_PAYLOAD = [("parent_hash", B(32)), ("fee_recipient", B(20)), ("state_root", B(32)), ("receipts_root", B(32)),
            ("logs_bloom", B(256)), ("prev_randao", B(32)), ("block_number", U64), ("gas_limit", U64),
            ("gas_used", U64), ("timestamp", U64), ("extra_data", BYTELIST(32)), ("base_fee_per_gas", U256),
            ("block_hash", B(32)), ("transactions", L(BYTELIST(2 ** 30), 2 ** 20))]
_BODY = [("randao_reveal", B(96)),
         ("eth1_data", C(("deposit_root", B(32)), ("deposit_count", U64), ("block_hash", B(32)))),
         ("graffiti", B(32)), ("proposer_slashings", L(PROPOSER_SLASHING, 16)),
         ("attester_slashings", L(ATTESTER_SLASHING, 2)), ("attestations", L(ATTESTATION, 128)),
         ("deposits", L(DEPOSIT, 16)), ("voluntary_exits", L(SIGNED_EXIT, 16))]


def signed_block_type(fork):
    body = list(_BODY)
    if fork >= 1:
        body.append(("sync_aggregate", SYNC_AGGREGATE))
    if fork == 2:
        body.append(("execution_payload", C(*_PAYLOAD)))
    if fork >= 3:
        body.append(("execution_payload", C(*_PAYLOAD, ("withdrawals", L(WITHDRAWAL, 16)))))
        body.append(("bls_to_execution_changes", L(SIGNED_BLS_CHANGE, 16)))
    block = C(("slot", U64), ("proposer_index", U64), ("parent_root", B(32)), ("state_root", B(32)),
              ("body", C(*body)))
    return C(("message", block), ("signature", B(96)))


def fixed_size(t):
    """byte size of a fixed-size type, None for a variable-size one"""
    k = t[0]
    if k == "u64":
        return 8
    if k == "u256":
        return 32
    if k == "bytes":
        return t[1]
    if k == "vector":
        return fixed_size(t[1]) * t[2]
    if k == "container":
        sizes = [fixed_size(ft) for _, ft in t[1]]
        return None if any(s is None for s in sizes) else sum(sizes)
    return None


def _hx(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


# ------------------------------------------------------------------ encode
def encode(t, v):
    k = t[0]
    if k == "u64":
        return int(v).to_bytes(8, "little")
    if k == "u256":
        return int(v).to_bytes(32, "little")
    if k == "bytes":
        b = _hx(v)
        assert len(b) == t[1], (len(b), t[1])
        return b
    if k in ("bytelist", "bitlist"):
        return _hx(v)
    if k == "vector":
        return b"".join(encode(t[1], x) for x in v)
    if k == "list":
        parts = [encode(t[1], x) for x in v]
        if fixed_size(t[1]) is not None:
            return b"".join(parts)
        off, table = 4 * len(parts), b""
        for p in parts:
            table += struct.pack("<I", off)
            off += len(p)
        return table + b"".join(parts)
    if k == "container":
        fixed, var = [], []
        for name, ft in t[1]:
            e = encode(ft, v[name])
            (fixed if fixed_size(ft) is not None else var).append(e)
            if fixed_size(ft) is None:
                fixed.append(None)
        off = sum(4 if f is None else len(f) for f in fixed)
        out, vi = b"", 0
        for f in fixed:
            if f is None:
                out += struct.pack("<I", off)
                off += len(var[vi])
                vi += 1
            else:
                out += f
        return out + b"".join(var)
    raise AssertionError(k)


def encode_signed_block(signed_block, fork):
    return encode(signed_block_type(fork), signed_block)


# ------------------------------------------------------------------ decode (strict)
def _offsets(data, at, count, lo):
    """`count` offsets read at the positions `at`: the first equals `lo`, none decreases, none passes the end"""
    offs = [struct.unpack_from("<I", data, p)[0] for p in at]
    if offs and offs[0] != lo:
        raise ValueError("first offset is not the end of the fixed part")
    for a, b in zip(offs, offs[1:] + [len(data)]):
        if a > b:
            raise ValueError("offset decreases or passes the end")
    return offs + [len(data)]


def decode(t, data):
    k = t[0]
    fs = fixed_size(t)
    if fs is not None and len(data) != fs:
        raise ValueError("wrong size")
    if k in ("u64", "u256"):
        return str(int.from_bytes(data, "little"))
    if k == "bytes":
        return "0x" + data.hex()
    if k == "bytelist":
        if len(data) > t[1]:
            raise ValueError("byte list over its limit")
        return "0x" + data.hex()
    if k == "bitlist":
        if not data or data[-1] == 0:
            raise ValueError("bitlist without its length bit")
        if 8 * (len(data) - 1) + data[-1].bit_length() - 1 > t[1]:
            raise ValueError("bitlist over its limit")
        return "0x" + data.hex()
    if k == "vector":
        n = fixed_size(t[1])
        return [decode(t[1], data[i * n:(i + 1) * n]) for i in range(t[2])]
    if k == "list":
        n = fixed_size(t[1])
        if n is not None:
            if len(data) % n or len(data) // n > t[2]:
                raise ValueError("list length")
            return [decode(t[1], data[i:i + n]) for i in range(0, len(data), n)]
        if not data:
            return []
        if len(data) < 4:
            raise ValueError("list shorter than an offset")
        first = struct.unpack_from("<I", data, 0)[0]
        if first == 0 or first % 4 or first > len(data) or first // 4 > t[2]:
            raise ValueError("first offset of a list")
        offs = _offsets(data, range(0, first, 4), first // 4, first)
        return [decode(t[1], data[a:b]) for a, b in zip(offs, offs[1:])]
    if k == "container":
        pos, at, fixed_end = 0, [], 0
        for _, ft in t[1]:
            fixed_end += 4 if fixed_size(ft) is None else fixed_size(ft)
        if len(data) < fixed_end:
            raise ValueError("container shorter than its fixed part")
        out, var = {}, []
        for name, ft in t[1]:
            n = fixed_size(ft)
            if n is None:
                at.append(pos)
                var.append((name, ft))
                pos += 4
            else:
                out[name] = decode(ft, data[pos:pos + n])
                pos += n
        offs = _offsets(data, at, len(at), fixed_end)
        for (name, ft), a, b in zip(var, offs, offs[1:]):
            out[name] = decode(ft, data[a:b])
        return {name: out[name] for name, _ in t[1]}
    raise AssertionError(k)


def decode_signed_block(data, fork):
    return decode(signed_block_type(fork), bytes(data))


def offset_words(t, data, base=0):
    """(position of the offset word, end of its container) for every offset in a valid encoding"""
    k = t[0]
    out = []
    if fixed_size(t) is not None or k in ("bytelist", "bitlist"):
        return out
    if k == "list":
        if not data or fixed_size(t[1]) is not None:
            return out
        first = struct.unpack_from("<I", data, 0)[0]
        offs = [struct.unpack_from("<I", data, p)[0] for p in range(0, first, 4)] + [len(data)]
        out += [(base + p, len(data)) for p in range(0, first, 4)]
        for a, b in zip(offs, offs[1:]):
            out += offset_words(t[1], data[a:b], base + a)
        return out
    pos, at, var = 0, [], []
    for name, ft in t[1]:
        if fixed_size(ft) is None:
            at.append(pos)
            var.append(ft)
            pos += 4
        else:
            pos += fixed_size(ft)
    offs = [struct.unpack_from("<I", data, p)[0] for p in at] + [len(data)]
    out += [(base + p, len(data)) for p in at]
    for ft, a, b in zip(var, offs, offs[1:]):
        out += offset_words(ft, data[a:b], base + a)
    return out


def hostile_corpus(data, fork):
    """[(label, bytes)]: every proper prefix of a valid encoding, and every offset word replaced in turn
    by 0, its value - 1 and + 1, its container's end, the end + 1 and 0xFFFFFFFF"""
    out = [("cut%d" % n, data[:n]) for n in range(len(data))]
    for pos, end in offset_words(signed_block_type(fork), data):
        v = struct.unpack_from("<I", data, pos)[0]
        for name, w in (("zero", 0), ("minus1", (v - 1) & 0xFFFFFFFF), ("plus1", v + 1), ("end", end),
                        ("end1", end + 1), ("ones", 0xFFFFFFFF)):
            if w != v:
                out.append(("off%d_%s" % (pos, name), data[:pos] + struct.pack("<I", w) + data[pos + 4:]))
    return out


# ------------------------------------------------------------------ what the rows must be
KINDS = ["randao", "proposer_slashing", "attester_slashing", "attestation", "voluntary_exit", "proposer",
         "sync_aggregate", "bls_to_execution_change"]


def _recording_state(gvr, prev_v, cur_v, fork_epoch, state_slot, fork):
    """a StateView whose keys are the references the device reports (lodestar_amd.signing_roots)"""
    from lodestar_amd import signing_roots as SR
    return SR.StateView(genesis_validators_root=gvr, fork_previous_version=prev_v, fork_current_version=cur_v,
                        fork_epoch=fork_epoch, pubkey=lambda i: ("index", i),
                        beacon_committee=lambda slot, index: ("committee", slot, index),
                        sync_committee=lambda: [("sync", i) for i in range(512)], slot=state_slot,
                        key_from_bytes=lambda b: ("bytes", bytes(b)), fork_seq=lambda slot: fork)


def expected_rows(signed_block, raw, fork, gvr, prev_v, cur_v, fork_epoch, state_slot, skip_proposer=False):
    """(status, rows, block root): rows = (kind, signing root, signature, ref) from the JSON of a block, by
    the parent's host walk for the set list and domains and by oracle/ssz.py for every object root.  `raw`
    (its encoding) gives the byte positions of the references.  status: "ok" or "verify_fail"."""
    import oracle.ssz as S
    from lodestar_amd import signing_roots as SR
    m = signed_block["message"]
    b = m["body"]
    st = _recording_state(gvr, prev_v, cur_v, fork_epoch, state_slot, fork)
    block_root = S.beacon_block(m, fork)
    st.beacon_committee = lambda slot, index: []  # an attestation's keys are not compared: its ref is
    try:
        sets = SR.block_signature_sets(signed_block, st, skip_proposer)
    except ValueError as e:
        assert "not infinity" in str(e)
        return "verify_fail", [], block_root

    def find(needle, start=0):
        p = raw.find(needle, start)
        assert p >= 0
        return p
    rows, n_at, n_sl, n_ps, n_ex, n_bc, cursor = [], 0, 0, 0, 0, 0, 0
    epoch = int(m["slot"]) // 32
    for s in sets:
        kind = KINDS.index(s.name)
        if s.name == "randao":
            obj, ref = S.uint64(epoch), (int(m["proposer_index"]), 0, 0, 0)
        elif s.name == "proposer_slashing":
            ps = b["proposer_slashings"][n_ps // 2]
            h = ps["signed_header_%d" % (n_ps % 2 + 1)]["message"]
            obj, ref = S.block_header(h), (int(ps["signed_header_1"]["message"]["proposer_index"]), 0, 0, 0)
            n_ps += 1
        elif s.name == "attester_slashing":
            ia = b["attester_slashings"][n_sl // 2]["attestation_%d" % (n_sl % 2 + 1)]
            enc = encode(INDEXED, ia)
            p = find(enc, cursor)
            cursor = p + len(enc)
            obj, ref = S.attestation_data(ia["data"]), (0, len(ia["attesting_indices"]), p + 228, len(enc) - 228)
            n_sl += 1
        elif s.name == "attestation":
            a = b["attestations"][n_at]
            enc = encode(ATTESTATION, a)
            p = find(enc, cursor)
            cursor = p + len(enc)
            obj = S.attestation_data(a["data"])
            ref = (int(a["data"]["slot"]), int(a["data"]["index"]), p + 228, len(enc) - 228)
            n_at += 1
        elif s.name == "voluntary_exit":
            e = b["voluntary_exits"][n_ex]["message"]
            obj, ref = S.voluntary_exit(e), (int(e["validator_index"]), 0, 0, 0)
            n_ex += 1
        elif s.name == "proposer":
            obj, ref = block_root, (int(m["proposer_index"]), 0, 0, 0)
        elif s.name == "sync_aggregate":
            obj = _hx(m["parent_root"])
            ref = (0, 0, find(encode(SYNC_AGGREGATE, b["sync_aggregate"])), 64)
        else:
            c = b["bls_to_execution_changes"][n_bc]
            p = find(encode(SIGNED_BLS_CHANGE, c), cursor)
            cursor = p + 172
            obj, ref = S.bls_to_execution_change(c["message"]), (0, 0, p + 8, 48)
            n_bc += 1
        # the domain the parent's walk chose is inside its signing tree: SigningData{object root, domain}
        domain = s.signing_root.parts[1]
        rows.append((kind, S.signing_root(obj, domain), bytes(s.signature), ref))
    return "ok", rows, block_root


DOMAIN_TYPES = ["00000000", "01000000", "02000000", "04000000", "07000000", "0a000000"]


def domains32(gvr, prev_v, cur_v):
    """2 x 6 x 32 bytes: [previous, current][proposer, attester, randao, voluntary_exit, sync, BLS change]"""
    import oracle.ssz as S
    return b"".join(S.compute_domain(bytes.fromhex(t), v, gvr) for v in (prev_v, cur_v) for t in DOMAIN_TYPES)


# ------------------------------------------------------------------ blocks
def _att_data(slot, index, salt):
    return {"slot": str(slot), "index": str(index), "beacon_block_root": "0x" + salt * 32,
            "source": {"epoch": str(slot // 32 - 1), "root": "0x" + "5a" * 32},
            "target": {"epoch": str(slot // 32), "root": "0x" + "5b" * 32}}


def bitlist_hex(n_bits, fill=0xA7):
    """an SSZ bitlist of n_bits bits (a pattern with set and clear bits), with its length bit"""
    v = 0
    for i in range(n_bits):
        if (fill >> (i % 8)) & 1 or i % 13 == 0:
            v |= 1 << i
    v |= 1 << n_bits
    return "0x" + v.to_bytes(n_bits // 8 + 1, "little").hex()


def attestation(slot, index, n_bits, salt="61"):
    return {"aggregation_bits": bitlist_hex(n_bits), "data": _att_data(slot, index, salt), "signature": "0x" + salt * 96}


def indexed(indices, slot, salt):
    return {"attesting_indices": [str(i) for i in indices], "data": _att_data(slot, 1, salt),
            "signature": "0x" + salt * 96}


def deposit(salt):
    return {"proof": ["0x" + ("%02x" % ((salt + i) & 255)) * 32 for i in range(33)],
            "data": {"pubkey": "0x" + "71" * 48, "withdrawal_credentials": "0x" + "72" * 32,
                     "amount": str(32 * 10 ** 9 + salt), "signature": "0x" + "73" * 96}}


def tx(n_bytes, salt=1):
    return "0x" + bytes((salt + 7 * i) & 255 for i in range(n_bytes)).hex()


def every_operation_block(k3):
    """the K3 capella block with every operation type: two proposer slashings, two attester slashings,
    three more attestations, two deposits, two exits, two BLS changes, transactions, extra_data"""
    blk = copy.deepcopy(k3["signed_block"])
    m = blk["message"]
    b = m["body"]
    slot = int(m["slot"])

    def header(pi, salt, s):
        return {"message": {"slot": str(s), "proposer_index": str(pi), "parent_root": "0x" + salt * 32,
                            "state_root": "0x" + "22" * 32, "body_root": "0x" + "33" * 32},
                "signature": "0x" + salt * 96}
    b["proposer_slashings"] = [{"signed_header_1": header(3, "a1", slot - 40), "signed_header_2": header(5, "a2", slot - 40)},
                               {"signed_header_1": header(6, "a3", 5), "signed_header_2": header(6, "a4", 5)}]
    b["attester_slashings"] = [
        {"attestation_1": indexed([1, 4, 9], slot - 3, "d1"), "attestation_2": indexed([4, 9, 20, 33, 61], slot - 3, "d2")},
        {"attestation_1": indexed([], 40, "d3"), "attestation_2": indexed(range(100, 237), 40, "d4")}]
    b["attestations"] = b["attestations"] + [attestation(slot - 1, 0, 0, "62"), attestation(slot - 2, 1, 257, "63"),
                                             attestation(70, 2, 2048, "64")]
    b["deposits"] = [deposit(1), deposit(90)]
    b["voluntary_exits"] = [{"message": {"epoch": "1", "validator_index": "7"}, "signature": "0x" + "b1" * 96},
                            {"message": {"epoch": str(slot // 32), "validator_index": "8"}, "signature": "0x" + "b2" * 96}]
    key48 = k3["state_view"]["validator_pubkeys48"][9]
    b["bls_to_execution_changes"] = [
        {"message": {"validator_index": str(v), "from_bls_pubkey": "0x" + key48, "to_execution_address": "0x" + a * 20},
         "signature": "0x" + a * 96} for v, a in ((9, "c1"), (11, "c3"))]
    b["execution_payload"]["extra_data"] = "0x" + "e7" * 5
    b["execution_payload"]["transactions"] = [tx(0), tx(1), tx(33, 3), tx(32 * 65, 5), tx(700, 9)]
    return blk


def fork_block(k3, fork):
    """one block per fork from the K3 block (capella) by dropping the later forks' fields; phase0 and altair
    keep its operations"""
    blk = copy.deepcopy(k3["signed_block"])
    b = blk["message"]["body"]
    if fork < 3:
        del b["bls_to_execution_changes"]
        del b["execution_payload"]["withdrawals"]
    if fork < 2:
        del b["execution_payload"]
    if fork < 1:
        del b["sync_aggregate"]
    return blk


def smallest_phase0_block():
    z = "0x" + "00" * 32
    return {"message": {"slot": "9", "proposer_index": "2", "parent_root": "0x" + "11" * 32, "state_root": "0x" + "12" * 32,
                        "body": {"randao_reveal": "0x" + "13" * 96,
                                 "eth1_data": {"deposit_root": z, "deposit_count": "0", "block_hash": z},
                                 "graffiti": z, "proposer_slashings": [], "attester_slashings": [], "attestations": [],
                                 "deposits": [], "voluntary_exits": []}},
            "signature": "0x" + "14" * 96}


# ------------------------------------------------------------------ tests/native/ssz_walk_check.cpp
def write_cases(path, cases):
    """cases: (fork, flags, fork_epoch, state_slot, domains (384 bytes), bytes)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for fork, flags, fork_epoch, state_slot, dom, raw in cases:
            assert len(dom) == 384
            f.write(struct.pack("<IIQQ", fork, flags, fork_epoch, state_slot) + dom + struct.pack("<I", len(raw)) + raw)


def parse_output(text):
    """[(status, block root, rows)] with rows as expected_rows gives them"""
    out, lines, i = [], text.splitlines(), 0
    while i < len(lines) and lines[i].startswith("case "):
        _, idx, status, n, root = lines[i].split()
        assert int(idx) == len(out)
        rows = []
        for ln in lines[i + 1:i + 1 + int(n)]:
            kind, r, sig, *ref = ln.split()
            rows.append((int(kind), bytes.fromhex(r), bytes.fromhex(sig), tuple(int(x) for x in ref)))
        out.append((int(status), bytes.fromhex(root), rows))
        i += 1 + int(n)
    assert lines[i] == "done %d" % len(out), lines[i:]
    return out


def canonical(v):
    """JSON with every number as the decimal string the beacon API (and decode) gives"""
    if isinstance(v, dict):
        return {k: canonical(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [canonical(x) for x in v]
    return str(v) if isinstance(v, int) else v
