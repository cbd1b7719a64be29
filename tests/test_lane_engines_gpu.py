"""The device arithmetic of the row engine (lb_row.h), the wave engine (lb_wave.h) and the 8-lane
program engine's reduction (lb_group_exec.h) at operand level: tools/ubench/lanes_check applies
the device functions to the records of tests/lane_engine_vectors.py, once, and every record's
output is compared here, in integers, with

  * the exact conditions (congruence mod p, the ranges the headers state, lanes 14 and 15 zero,
    canonical outputs byte for byte), the same functions tests/test_lane_engine_vectors_cpu.py
    holds the models to;
  * the models limb for limb (tools/gen_row_programs.py rp_mul / lin / norm,
    tools/gen_wave_programs.py quotient_estimate), which the headers say mirror the device exactly;
  * at the Fp12 level, oracle/bls_oracle.py's tower, and the other engine's bytes.

There is no tolerance anywhere.  A failure names the operation and the classes of its records."""
import json
import os
import subprocess

import pytest

import lane_engine_vectors as V

pytestmark = pytest.mark.gpu

R, G, P = V.R, V.G, V.P
EXE = os.path.join(V.ROOT, "tools", "ubench", "lanes_check")


def run_carrier(exe, recs, workdir):
    """one run of the carrier over every record; op name -> output words per record"""
    inp, outp = os.path.join(workdir, "lanes_in.bin"), os.path.join(workdir, "lanes_out.bin")
    with open(inp, "wb") as f:
        f.write(V.pack_input(recs))
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, "lanes_check exit %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    counts = json.loads(p.stdout.strip().splitlines()[-1])
    assert counts == {name: len(rs) for name, rs in recs.items()}
    with open(outp, "rb") as f:
        return V.parse_output(f.read(), recs)


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    recs = V.all_records()
    return recs, run_carrier(EXE, recs, str(tmp_path_factory.mktemp("lanes")))


class Problems:
    """what went wrong, by operation and class (every record is looked at; none is skipped)"""

    def __init__(self):
        self.by, self.first, self.seen = {}, [], 0

    def look(self, name, i, rec, err):
        self.seen += 1
        if err is not None:
            self.by[(name, rec.cls)] = self.by.get((name, rec.cls), 0) + 1
            if len(self.first) < 6:
                self.first.append("%s[%d] (%s): %s" % (name, i, rec.cls, err))

    def report(self):
        classes = ", ".join("%s/%s x%d" % (n, c, k) for (n, c), k in sorted(self.by.items()))
        return "failing classes: %s\n%s" % (classes, "\n".join(self.first))


def _same_limbs(got, want):
    if got == want:
        return None
    return "differs from the model in limbs %r: device %r, model %r" % (
        [k for k in range(16) if got[k] != want[k]], got, want)


def check_row_products(recs, out):
    pr = Problems()
    for name in ("rp_mul", "r1_mul", "r1_sqr", "f_mul"):
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            r = V.signed(w)
            pr.look(name, i, rec, V.exact_row_product(rec.x, rec.y, r) or _same_limbs(r, R.rp_mul(rec.x, rec.y)))
    return pr


def check_row_sums(recs, out):
    pr = Problems()
    for i, (rec, w) in enumerate(zip(recs["r_reduce"], out["r_reduce"])):
        r = V.signed(w)
        pr.look("r_reduce", i, rec, V.exact_row_sum(rec.v, r, True) or _same_limbs(r, R.lin([(1, rec.acc)])))
    for name, red in (("r_operand_carry", False), ("r_operand_red", True)):
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            r = V.signed(w)
            pr.look(name, i, rec, V.exact_row_sum(rec.v, r, red) or _same_limbs(r, R.lin(rec.terms, reduce=red)))
    for name in V.RFP_TERMS:
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            r, t = V.signed(w), V.rfp_terms(name, rec)
            v = sum(c * R.val(l) for c, l in t)
            pr.look(name, i, rec, V.exact_row_sum(v, r, True) or _same_limbs(r, R.lin(t)))
    return pr


def _same_words(got, want, what):
    return None if got == want else "%s: device %x, expected %x" % (what, V.fp_of_words(got), V.fp_of_words(want))


def check_canonical(recs, out):
    pr = Problems()
    for i, (rec, w) in enumerate(zip(recs["r_canon"], out["r_canon"])):
        pr.look("r_canon", i, rec, _same_words(w, V.fp_words(rec.v % P), "v mod p"))
    for name in ("r_export", "r1_export"):
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            pr.look(name, i, rec, _same_words(w, V.export_expected(rec.v), "v / 2^8 mod p"))
    for i, (rec, w) in enumerate(zip(recs["r_import_export"], out["r_import_export"])):
        slot, raw = V.signed(w[:16]), R.limbs(rec.a << 8)
        pr.look("r_import_export", i, rec, V.exact_row_sum(rec.a << 8, slot, True) or _same_limbs(slot, R.lin([(1, raw)]))
                or _same_words(w[16:], V.fp_words(rec.a), "import then export"))
    for i, (rec, w) in enumerate(zip(recs["r1_import_export"], out["r1_import_export"])):
        pr.look("r1_import_export", i, rec, _same_limbs(V.signed(w[:16]), R.limbs(rec.a << 8))
                or _same_words(w[16:], V.fp_words(rec.a), "import then export"))
    return pr


def check_wave_sums(recs, out):
    pr = Problems()
    for name in ("w_lin_maxp", "w_lin_maxp_full", "w_lin_maxl", "w_lin_maxl_full", "g_reduce", "g_reduce_full"):
        full = name.endswith("_full")
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            pr.look(name, i, rec, V.exact_wave_sum(rec.v, w, full)
                    or _same_words(w, V.fp_words(V.model_wave_sum(rec, full)), "V - (q - 1) p of the model"))
    return pr


_EXPECT = {}


def _f12_expected(op, rec):
    """the oracle's result of an Fp12-level operation, computed once per record"""
    from oracle import bls_oracle as o
    key = (op, id(rec))
    if key not in _EXPECT:
        a = V.f12_tower(rec.a)
        if op == "mul":
            v = o.f12_mul(a, V.f12_tower(rec.b))
        elif op in ("sqr", "csqr"):
            v = o.f12_sqr(a)
        elif op == "frob":
            v = o.f12_pow(a, P)
        elif op == "frob2":
            v = o.f12_pow(a, P * P)
        elif op == "conj":
            v = o.f12_conj(a)
        else:
            v = o.f12_inv(a)
        _EXPECT[key] = V.f12_flat(v)
    return _EXPECT[key]


def _same_f12(w, want):
    got = V.f12_of_words(w)
    if any(V.fp_of_words(w[12 * k:12 * k + 12]) >= P for k in range(12)):
        return "a coefficient is not below p"
    if got != want:
        return "differs from the oracle in coefficients %r" % [k for k in range(12) if got[k] != want[k]]
    return None


def check_fp12(recs, out):
    pr = Problems()
    for name in ("r_mul", "r_sqr", "r_csqr", "r_frob", "r_frob2", "w_mul", "w_sqr", "w_frob", "w_frob2", "w_conj", "w_inv"):
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            pr.look(name, i, rec, _same_f12(w, _f12_expected(name[2:], rec)))
    for op in ("mul", "sqr", "frob", "frob2", "is_one"):  # the two engines: the same bytes
        for i, rec in enumerate(recs["r_" + op]):
            same = out["r_" + op][i] == out["w_" + op][i]
            pr.look("r_%s / w_%s" % (op, op), i, rec, None if same else "the row and the wave engine differ")
    seen = {}
    for name in ("r_is_one", "w_is_one", "r_eq"):
        for i, (rec, w) in enumerate(zip(recs[name], out[name])):
            want = (rec.a == rec.b) if name == "r_eq" else (rec.a == [1] + [0] * 11)
            seen.setdefault(name, set()).add(want)
            pr.look(name, i, rec, None if w == [1 if want else 0] else "device %r, expected %r" % (w, want))
    assert all(s == {True, False} for s in seen.values()), seen
    return pr


def check_pdbl(recs, out):
    from oracle import bls_oracle as o
    pr = Problems()
    for i, (rec, w) in enumerate(zip(recs["r_pdbl_fast"], out["r_pdbl_fast"])):
        c = [V.unmont(V.fp_of_words(w[12 * k:12 * k + 12])) for k in range(6)]
        X, Y, Z = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
        want = rec.point
        for _ in range(rec.chain):
            want = o.g2_add(want, want)
        err = None
        if any(V.fp_of_words(w[12 * k:12 * k + 12]) >= P for k in range(6)):
            err = "a coordinate is not below p"
        elif Z == (0, 0):
            err = "Z = 0"
        else:
            zi = o.f2_inv(Z)
            if (o.f2_mul(X, zi), o.f2_mul(Y, zi)) != want:
                err = "not 2^%d P" % rec.chain
        pr.look("r_pdbl_fast", i, rec, err)
    return pr


CHECKS = {"row_products": (check_row_products, ("rp_mul", "r1_mul", "r1_sqr", "f_mul")),
          "row_sums": (check_row_sums, ("r_reduce", "r_operand_carry", "r_operand_red") + tuple(V.RFP_TERMS)),
          "canonical": (check_canonical, ("r_canon", "r_export", "r1_export", "r_import_export", "r1_import_export")),
          "wave_sums": (check_wave_sums, ("w_lin_maxp", "w_lin_maxp_full", "w_lin_maxl", "w_lin_maxl_full", "g_reduce",
                                          "g_reduce_full")),
          "fp12": (check_fp12, ("r_mul", "r_sqr", "r_csqr", "r_frob", "r_frob2", "r_is_one", "r_eq", "w_mul", "w_sqr",
                                "w_frob", "w_frob2", "w_conj", "w_inv", "w_is_one")),
          "pdbl": (check_pdbl, ("r_pdbl_fast",))}


def _run_check(lanes, family):
    recs, out = lanes
    fn, names = CHECKS[family]
    pr = fn(recs, out)
    assert pr.seen >= sum(len(recs[n]) for n in names)  # no record skipped
    assert not pr.by, pr.report()


def test_every_operation_belongs_to_a_family():
    assert sorted(n for _, names in CHECKS.values() for n in names) == sorted(V.OPS)


def test_row_products(lanes):
    """rp_mul, r1_mul, r1_sqr, f_mul: x y / 2^392 (mod p) within |x y| / 2^392 + 1.0001 p, limbs
    in the slot range, lanes 14 and 15 zero; equal to the model's rp_mul limb for limb"""
    _run_check(lanes, "row_products")


def test_row_sums(lanes):
    """r_reduce, r_operand (carry-only and reduced), f_add / f_sub / f_neg / f_mul3 / f_mul8: the
    exact sum (carry-only) or congruent within [-p / 2^20, p + p / 2^20); equal to the model's lin"""
    _run_check(lanes, "row_sums")


def test_canonical_forms_import_and_export(lanes):
    """r_canon, r_export, r1_export: the canonical words of the Python integer mod p; the staged
    and the one-row import followed by export give the value back, the imported slot as the model's"""
    _run_check(lanes, "canonical")


def test_wave_and_group_sums(lanes):
    """w_lin<LBW_MAXP>, w_lin<LBW_MAXL>, g_reduce, full 0 and 1: congruent, in [0, 3p) (below p
    when full), and equal to V - (quotient_estimate - 1) p of the model"""
    _run_check(lanes, "wave_sums")


def test_fp12_operations_of_both_engines(lanes):
    """products, squarings, Frobenius maps, conjugate, inverse against the oracle's tower; the row
    and the wave engine byte-identical; is_one / eq true and false"""
    _run_check(lanes, "fp12")


def test_projective_doubling_chain(lanes):
    """r_pdbl_fast chained 1, 2 and 70 times from a random projective representation"""
    _run_check(lanes, "pdbl")
