#!/usr/bin/env python3
"""Generates tests/golden/edge_points.json from the CPU oracle: point encodings an attacker can
pick freely, for every decode path (g2_decompress96_w / _wp, g1_decompress48, g1_deserialize96).

Each record: name, kind (g2c96: 96-byte compressed G2; g1c48: 48-byte compressed G1; g1u96:
96-byte uncompressed G1), hex, status (the oracle's decode without a subgroup check: ok / inf / a
BLST_* name), status_validated (Signature.fromBytes(validate=true) for G2; PublicKey.keyValidate
for G1, where an infinity key is BLST_PK_IS_INFINITY), point (the decoded affine point in the
library's uncompressed byte order, G1 x || y, G2 x.c1 || x.c0 || y.c1 || y.c0; null where nothing
decodes or at infinity), tags.  G2 records carry verify as well: the verdict of the one-set job
(pubkey96, signing_root, that signature) as oracle.verify_job gives it.

G2 x values whose x^3 + 4(1+i) has a zero component, which no honest signature has, reach the
special branches of the Fp2 square root and of the sign choice:
  rhs_in_Fp_qr     x = (a, b) with 3 a^2 b - b^3 + 4 = 0 and rhs.c0 a residue: y = (s, 0)
                   (tag y_c1_zero: the sign is decided by y.c0)
  rhs_in_Fp_nonqr  the same with rhs.c0 a non-residue: alpha = -rhs.c0, (rhs.c0 + alpha)/2 = 0
                   (tag d1_zero) and y = (0, s) (tag y_c0_zero)
  rhs_imag         a^3 - 3 a b^2 + 4 = 0 (tag rhs_c0_zero)

Run from the repo root:
    python3 tests/golden/make_edge_points.py
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls_oracle as o  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "edge_points.json")
P = o.P
H1 = (o.BLS_X - 1) ** 2 // 3      # cofactor of G1 in E1(Fp): 3 * 11^2 * 10177^2 * ...
KEY_INDEX = 7                     # the interop key the valid records belong to
KEY_ROOT = bytes([0xE7]) * 32     # ... and the root its signature is over
STATUSES = ("ok", "inf", "BLST_BAD_ENCODING", "BLST_POINT_NOT_ON_CURVE", "BLST_POINT_NOT_IN_GROUP")


def b48(v):
    return v.to_bytes(48, "big")


def g2_raw(x1, x0, flags=0x80):
    """96 bytes x.c1 || x.c0 of any two integers below 2^381 / 2^384, with flag bits"""
    b = bytearray(b48(x1) + b48(x0))
    assert b[0] & 0xE0 == 0
    b[0] |= flags
    return bytes(b)


def with_flags(body, flags):
    return bytes([(body[0] & 0x1F) | flags]) + body[1:]


def g2_rhs(x):
    return o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2)


def g2_status(b):
    try:
        pt = o.g2_decompress(b)
        st = "inf" if pt is None else "ok"
    except o.BlsError as e:
        return str(e), str(e), None
    try:
        o.signature_from_bytes(b, True)
        stv = st
    except o.BlsError as e:
        stv = str(e)
    pthex = None if pt is None else (b48(pt[0][1]) + b48(pt[0][0]) + b48(pt[1][1]) + b48(pt[1][0])).hex()
    return st, stv, pthex


def g1_status(b):
    try:
        pt = o.g1_deserialize(b)
        st = "inf" if pt is None else "ok"
    except o.BlsError as e:
        return str(e), str(e), None
    if pt is None:
        stv = "BLST_PK_IS_INFINITY"
    else:
        stv = "ok" if o.g1_mul(pt, o.R) is None else "BLST_POINT_NOT_IN_GROUP"
    return st, stv, None if pt is None else o.g1_serialize(pt).hex()


def main(out_path=OUT):
    rnd = random.Random(0x45444745)
    recs = []
    sk = o.interop_secret_key(KEY_INDEX)
    pk = o.sk_to_pk(sk)
    pk96 = o.g1_serialize(pk)
    sig = o.sign(sk, KEY_ROOT)

    def g2(name, b, tags=()):
        st, stv, pt = g2_status(b)
        if stv == "ok":
            verify = o.verify_job([([pk96], KEY_ROOT, b)])
        else:
            verify = False if stv == "inf" else stv
        recs.append({"name": name, "kind": "g2c96", "hex": b.hex(), "status": st, "status_validated": stv,
                     "verify": verify, "point": pt, "tags": sorted(tags)})
        return recs[-1]

    def g1(name, b, tags=()):
        st, stv, pt = g1_status(b)
        recs.append({"name": name, "kind": "g1c48" if len(b) == 48 else "g1u96", "hex": b.hex(), "status": st,
                     "status_validated": stv, "point": pt, "tags": sorted(tags)})
        return recs[-1]

    # ------------------------------------------------------------------ G2: rhs with a zero component
    def x_rhs_in_fp(want_qr):
        while True:
            b = rnd.randrange(1, P)
            a = o.fp_sqrt((b * b * b - 4) * o.fp_inv(3 * b))
            if a is None:
                continue
            rhs = g2_rhs((a, b))
            assert rhs[1] == 0
            if rhs[0] != 0 and o.fp_is_square(rhs[0]) == want_qr:
                return (a, b)

    def x_rhs_imag():
        while True:
            a = rnd.randrange(1, P)
            b = o.fp_sqrt((a * a * a + 4) * o.fp_inv(3 * a))
            if b is None:
                continue
            rhs = g2_rhs((a, b))
            assert rhs[0] == 0
            if rhs[1] != 0 and o.f2_sqrt(rhs) is not None:
                return (a, b)

    def d1_is_zero(rhs):
        alpha = pow((rhs[0] * rhs[0] + rhs[1] * rhs[1]) % P, (P + 1) // 4, P)   # the device's candidate
        return (rhs[0] + alpha) % P == 0

    for cls, draw, tags in (("rhs_in_Fp_qr", lambda: x_rhs_in_fp(True), {"y_c1_zero"}),
                            ("rhs_in_Fp_nonqr", lambda: x_rhs_in_fp(False), {"y_c0_zero", "d1_zero"}),
                            ("rhs_imag", x_rhs_imag, {"rhs_c0_zero"})):
        for k in range(2):
            x = draw()
            rhs = g2_rhs(x)
            for sign in (0, 1):
                r = g2(f"{cls}_{k}_sign{sign}", g2_raw(x[1], x[0], 0x80 | (0x20 if sign else 0)), tags | {cls})
                assert r["status"] == "ok" and r["status_validated"] == "BLST_POINT_NOT_IN_GROUP", r
                y = o.g2_decompress(bytes.fromhex(r["hex"]))[1]
                assert ("y_c1_zero" in tags) == (y[1] == 0) and ("y_c0_zero" in tags) == (y[0] == 0)
                assert ("d1_zero" in tags) == d1_is_zero(rhs) and ("rhs_c0_zero" in tags) == (rhs[0] == 0)
                assert o.g2_compress((x, y)) == bytes.fromhex(r["hex"])
                if "y_c1_zero" in tags:
                    assert (y[0] > o.HALF_P) == bool(sign)

    # ------------------------------------------------------------------ G2: fixed x
    on_curve = {(0, 0): False, (1, 0): False, (0, P - 1): False, (2, 0): True, (0, 1): True, (P - 1, 0): True,
                (P - 1, P - 1): True}
    for x in ((0, 0), (1, 0), (2, 0), (0, 1), (P - 1, 0), (P - 1, P - 1), (0, P - 1)):
        nm = "x_" + "_".join("pm1" if c == P - 1 else str(c) for c in x)
        for sign in (0, 1):
            r = g2(f"{nm}_sign{sign}", g2_raw(x[1], x[0], 0x80 | (0x20 if sign else 0)), {"fixed_x"})
            want = ("ok", "BLST_POINT_NOT_IN_GROUP") if on_curve[x] else ("BLST_POINT_NOT_ON_CURVE",) * 2
            assert (r["status"], r["status_validated"]) == want, r

    # ------------------------------------------------------------------ G2: bad encodings, flag bytes
    sigb = o.g2_compress(sig)
    sx1, sx0 = int.from_bytes(with_flags(sigb, 0)[:48], "big"), int.from_bytes(sigb[48:], "big")
    sflags = sigb[0] & 0xE0
    assert sx0 < 2 ** 384 - P
    for name, b in (("bad_x_c1_eq_p", g2_raw(P, sx0, sflags)), ("bad_x_c0_eq_p", g2_raw(sx1, P, sflags)),
                    ("bad_x_c0_all_ones", g2_raw(sx1, 2 ** 384 - 1, sflags)),
                    ("bad_x_c0_plus_p", g2_raw(sx1, sx0 + P, sflags))):
        r = g2(name, b, {"bad_encoding"})
        assert r["status"] == "BLST_BAD_ENCODING", r
    for fl in (0x00, 0x20, 0x40):
        r = g2("flag_%02x_valid_body" % fl, with_flags(sigb, fl), {"flags"})
        assert r["status"] == "BLST_BAD_ENCODING", r
    r = g2("flag_c0_zeros", bytes([0xC0]) + bytes(95), {"flags", "infinity"})
    assert (r["status"], r["status_validated"], r["verify"]) == ("inf", "inf", False)
    for name, b in (("flag_e0_zeros", bytes([0xE0]) + bytes(95)), ("flag_c0_last_byte_1", bytes([0xC0]) + bytes(94) + b"\x01"),
                    ("flag_c0_byte_47", bytes([0xC0]) + bytes(46) + b"\x01" + bytes(48))):
        r = g2(name, b, {"flags"})
        assert r["status"] == "BLST_BAD_ENCODING", r

    # ------------------------------------------------------------------ G2: valid signatures and negations
    r = g2("valid_sig_key", sigb, {"valid"})
    assert (r["status_validated"], r["verify"]) == ("ok", True)
    r = g2("valid_sig_key_negated", o.g2_compress(o.g2_neg(sig)), {"valid", "negated"})
    assert (r["status_validated"], r["verify"]) == ("ok", False) and bytes.fromhex(r["hex"]) == with_flags(sigb, sflags ^ 0x20)
    other = o.sign(o.interop_secret_key(KEY_INDEX + 1), bytes([0xE8]) * 32)   # valid, but of another key and root
    for name, s in (("valid_sig_other", other), ("valid_sig_other_negated", o.g2_neg(other))):
        r = g2(name, o.g2_compress(s), {"valid", "other_key"})
        assert (r["status_validated"], r["verify"]) == ("ok", False)

    # ------------------------------------------------------------------ G1 points
    def curve_point():
        while True:
            x = rnd.randrange(P)
            y = o.fp_sqrt(x * x * x + o.B1)
            if y is not None:
                return (x, y)

    assert H1 % 121 == 0 and o.g1_mul(curve_point(), o.R * H1) is None
    while True:
        q11 = o.g1_mul(curve_point(), o.R * H1 // 121)
        if q11 is not None:
            if o.g1_mul(q11, 11) is not None:
                q11 = o.g1_mul(q11, 11)
            break
    assert q11 is not None and o.g1_mul(q11, 11) is None
    t3 = (0, 2)
    assert o.g1_on_curve(t3) and o.g1_mul(t3, 3) is None
    mixed = o.g1_add(o.sk_to_pk(7), t3)
    assert o.g1_on_curve(mixed) and o.g1_mul(mixed, o.R) is not None
    x_off = next(x for x in range(2, 100) if o.fp_sqrt(x * x * x + o.B1) is None)
    small = next(q for q in (o.sk_to_pk(o.interop_secret_key(i)) for i in range(64))
                 if q[0] < 2 ** 381 - P)                                           # x + p fits under the flag bits
    assert o.fp_sqrt(3) is None                                                    # x = p - 1: rhs = 3, off the curve
    points = [("key", pk, {"valid", "key"}), ("key_negated", o.g1_neg(pk), {"valid", "neg_key"}),
              ("order3", t3, {"order3", "outside_g1"}), ("order3_negated", o.g1_neg(t3), {"order3", "outside_g1"}),
              ("order11", q11, {"order11", "outside_g1"}), ("key7_plus_order3", mixed, {"mixed", "outside_g1"})]

    # 48-byte
    kb = o.g1_compress(pk)
    for name, pt, tags in points:
        b = o.g1_compress(pt)
        r = g1(name, b, tags)
        want = "ok" if "valid" in tags else "BLST_POINT_NOT_IN_GROUP"
        assert (r["status"], r["status_validated"]) == ("ok", want), r
    assert bytes.fromhex(recs[-len(points)]["hex"]) == with_flags(kb, kb[0] & 0xE0)
    assert bytes.fromhex(recs[-len(points) + 1]["hex"]) == with_flags(kb, (kb[0] & 0xE0) ^ 0x20)      # both sign bits
    assert {bytes.fromhex(rr["hex"])[0] for rr in recs if "order3" in rr["tags"]} == {0x80, 0xA0}
    r = g1("x_pm1", with_flags(b48(P - 1), 0x80), {"off_curve"})
    assert r["status"] == "BLST_POINT_NOT_ON_CURVE", r
    r = g1("x_off_curve", with_flags(b48(x_off), 0x80), {"off_curve"})
    assert r["status"] == "BLST_POINT_NOT_ON_CURVE", r
    for name, v in (("bad_x_eq_p", P), ("bad_x_all_ones", 2 ** 381 - 1), ("bad_x_plus_p", small[0] + P)):
        r = g1(name, with_flags(b48(v), 0x80 | (o.g1_compress(small)[0] & 0x20)), {"bad_encoding"})
        assert r["status"] == "BLST_BAD_ENCODING", r
    for fl in (0x00, 0x40):
        r = g1("flag_%02x_valid_body" % fl, with_flags(kb, fl), {"flags"})
        assert r["status"] == "BLST_BAD_ENCODING", r
    r = g1("flag_c0_zeros", bytes([0xC0]) + bytes(47), {"flags", "infinity"})
    assert (r["status"], r["status_validated"]) == ("inf", "BLST_PK_IS_INFINITY")
    for name, b in (("flag_e0_zeros", bytes([0xE0]) + bytes(47)), ("flag_c0_nonzero_tail", bytes([0xC0]) + bytes(46) + b"\x01")):
        r = g1(name, b, {"flags"})
        assert r["status"] == "BLST_BAD_ENCODING", r

    # 96-byte
    for name, pt, tags in points:
        r = g1(name, o.g1_serialize(pt), tags)
        want = "ok" if "valid" in tags else "BLST_POINT_NOT_IN_GROUP"
        assert (r["status"], r["status_validated"]) == ("ok", want), r
    x, y = pk
    assert b48(x) + b48(P - y) == o.g1_serialize(o.g1_neg(pk))           # (x, p - y) is key_negated above
    for name, b, want, tags in (
            ("x_off_curve", b48(x_off) + b48(1), "BLST_POINT_NOT_ON_CURVE", {"off_curve"}),
            ("x_pm1", b48(P - 1) + b48(1), "BLST_POINT_NOT_ON_CURVE", {"off_curve"}),
            ("y_plus_1", b48(x) + b48(y + 1), "BLST_POINT_NOT_ON_CURVE", {"off_curve"}),
            ("bad_x_eq_p", b48(P) + b48(2), "BLST_BAD_ENCODING", {"bad_encoding"}),
            ("bad_x_all_ones", b48(2 ** 381 - 1) + b48(y), "BLST_BAD_ENCODING", {"bad_encoding"}),
            ("bad_x_plus_p", b48(small[0] + P) + b48(small[1]), "BLST_BAD_ENCODING", {"bad_encoding"}),
            ("bad_y_plus_p", b48(x) + b48(y + P), "BLST_BAD_ENCODING", {"bad_encoding"}),
            ("bad_y_eq_p", b48(0) + b48(P), "BLST_BAD_ENCODING", {"bad_encoding"}),
            ("flag_20_valid_body", with_flags(pk96, 0x20), "BLST_BAD_ENCODING", {"flags", "flag_20"}),
            ("flag_80_valid_body", with_flags(pk96, 0x80), "BLST_BAD_ENCODING", {"flags"}),
            ("flag_40_nonzero_tail", bytes([0x40]) + bytes(94) + b"\x01", "BLST_BAD_ENCODING", {"flags"}),
            ("flag_60_zeros", bytes([0x60]) + bytes(95), "BLST_BAD_ENCODING", {"flags"})):
        r = g1(name, b, tags)
        assert r["status"] == want, r
    r = g1("flag_40_zeros", bytes([0x40]) + bytes(95), {"flags", "infinity"})
    assert (r["status"], r["status_validated"]) == ("inf", "BLST_PK_IS_INFINITY")

    # every status occurs per kind where it can
    for kind in ("g2c96", "g1c48", "g1u96"):
        mine = [r for r in recs if r["kind"] == kind]
        assert len({r["name"] for r in mine}) == len(mine)
        assert {r["status"] for r in mine} == set(STATUSES) - {"BLST_POINT_NOT_IN_GROUP"}, kind
        want = set(STATUSES) - ({"inf"} if kind != "g2c96" else set()) | ({"BLST_PK_IS_INFINITY"} if kind != "g2c96" else set())
        assert {r["status_validated"] for r in mine} == want, kind
    assert len([r for r in recs if r["kind"] == "g2c96"]) <= 64      # the GPU tests pad them to 65 groups

    out = {"generator": "tests/golden/make_edge_points.py",
           "note": "adversarial point encodings; statuses, points and verdicts are the oracle's. verify is the "
                   "verdict of the one-set job (key.pubkey96, key.signing_root, the record's signature)",
           "key": {"interop_index": KEY_INDEX, "pubkey96": pk96.hex(), "pubkey48": kb.hex(),
                   "signing_root": KEY_ROOT.hex(), "signature": sigb.hex()},
           "records": recs}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:2])
