"""Operand-level vectors for the row, wave and group engines (lb_row.h, lb_wave.h,
lb_group_exec.h), built from Python integers: deterministic (seeded), every record in a named
class.  tools/ubench/lanes_check applies the device functions to them (its header documents the
file layout that pack_input writes); tests/test_lane_engine_vectors_cpu.py checks with the models
alone that the vectors mean something, tests/test_lane_engines_gpu.py checks the device.

A record is a Rec: .cls (its class), .words (the input words) and the Python integers it was
built from (.x, .y, .terms, ...), which the tests compute the exact results from."""
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gen_row_programs as R  # noqa: E402
import gen_wave_programs as G  # noqa: E402

P, RP, M28 = R.P, R.RP, R.M28
B28 = 1 << 28
EDGE = (-1, 0, 1, B28 - 1, B28, B28 + 1)
MAGIC = 0x4C414E45
MAXP, MAXL = G.MAXP, G.MAXL
MAX_RECORDS = 4096
PDBL_CHAIN = 70
# the d of v = k p + d
DS = [0, 1, -1, 2, -2, 1 << 20, -(1 << 20), P >> 30, -(P >> 30), (P - 1) // 2, -((P - 1) // 2)]

# op name -> (id, input words, output words): tools/ubench/lanes_check.hip's table
OPS = {
    "rp_mul": (1, 28, 16), "r1_mul": (2, 28, 16), "r1_sqr": (3, 14, 16), "r_reduce": (4, 32, 16),
    "f_add": (5, 28, 16), "f_sub": (6, 28, 16), "f_neg": (7, 28, 16), "f_mul3": (8, 28, 16),
    "f_mul8": (9, 28, 16), "f_mul": (10, 28, 16),
    "r_operand_carry": (11, 121, 16), "r_operand_red": (12, 121, 16),
    "r_canon": (13, 14, 12), "r_export": (14, 14, 12), "r_import_export": (15, 12, 28),
    "r1_import_export": (16, 12, 28), "r1_export": (17, 14, 12),
    "w_lin_maxp": (20, 2 + 13 * MAXP, 12), "w_lin_maxp_full": (21, 2 + 13 * MAXP, 12),
    "w_lin_maxl": (22, 2 + 13 * MAXL, 12), "w_lin_maxl_full": (23, 2 + 13 * MAXL, 12),
    "g_reduce": (24, 48, 12), "g_reduce_full": (25, 48, 12),
    "r_mul": (30, 288, 144), "r_sqr": (31, 144, 144), "r_csqr": (32, 144, 144), "r_frob": (33, 144, 144),
    "r_frob2": (34, 144, 144), "r_is_one": (35, 144, 1), "r_eq": (36, 288, 1), "r_pdbl_fast": (37, 73, 72),
    "w_mul": (40, 288, 144), "w_sqr": (41, 144, 144), "w_frob": (42, 144, 144), "w_frob2": (43, 144, 144),
    "w_conj": (44, 144, 144), "w_inv": (45, 144, 144), "w_is_one": (46, 144, 1),
}


class Rec:
    def __init__(self, cls, words, **kw):
        self.cls, self.words = cls, words
        self.__dict__.update(kw)


# ------------------------------------------------------------ words
def u32(x):
    return x & 0xFFFFFFFF


def i64_words(x):
    assert -(1 << 63) <= x < (1 << 63)
    return [x & 0xFFFFFFFF, (x >> 32) & 0xFFFFFFFF]


def fp_words(x):
    """12 words of an integer below 2^384"""
    assert 0 <= x < (1 << 384)
    return [(x >> (32 * j)) & 0xFFFFFFFF for j in range(12)]


def fp_of_words(w):
    return sum(v << (32 * j) for j, v in enumerate(w))


def mont(x):
    """the 2^384-Montgomery value of a field element (what an `fp` holds)"""
    return x * (1 << 384) % P


def unmont(v):
    return v * pow(1 << 384, -1, P) % P


def limb_words(l):
    for x in l[:14]:
        assert -(1 << 31) <= x < (1 << 31)
    return [u32(x) for x in l[:14]]


def signed(words):
    return [w - (1 << 32) if w >= (1 << 31) else w for w in words]


# ------------------------------------------------------------ limb spellings
def edge_slot(rnd, bound, sign=0, p_random=0.3, odd=False):
    """limbs 0..12 drawn from {-1, 0, 1, 2^28 - 1, 2^28, 2^28 + 1, random}, a signed top limb
    that puts the value inside (-bound, bound) (sign: +1 / -1 forces it)"""
    while True:
        l = [rnd.randrange(B28) if rnd.random() < p_random else rnd.choice(EDGE) for _ in range(13)]
        if odd:
            l[0] = rnd.choice((-1, 1, B28 - 1, B28 + 1, rnd.randrange(B28) | 1))
        low = sum(v << (28 * k) for k, v in enumerate(l))
        tmin = -((bound - 1 + low) >> 364)          # ceil((-bound + 1 - low) / 2^364)
        tmax = (bound - 1 - low) >> 364
        if sign > 0:
            tmin = max(tmin, 1)
        if sign < 0:
            tmax = min(tmax, -2)
        if tmin > tmax:
            continue
        t = rnd.randint(tmin, tmax)
        out = l + [t, 0, 0]
        assert abs(R.val(out)) < bound
        return out


def respell(l, rnd, p=0.5):
    """the same value in other limbs of the slot range [-1, 2^28 + 2): a limb of 0 or 1 borrows
    2^28 from the next one, a limb of 2^28 - 1 lends it"""
    l = list(l)
    for k in range(13):
        if rnd.random() >= p:
            continue
        nxt_lo = -(1 << 30) if k == 12 else -1
        nxt_hi = (1 << 30) if k == 12 else B28 + 1
        if l[k] in (0, 1) and l[k + 1] - 1 >= nxt_lo:
            l[k] += B28
            l[k + 1] -= 1
        elif l[k] == B28 - 1 and l[k + 1] + 1 <= nxt_hi:
            l[k] -= B28
            l[k + 1] += 1
    return l


def edgy_value(rnd, lo, hi):
    """an integer in [lo, hi] many of whose canonical limbs are 0, 1 or 2^28 - 1"""
    while True:
        l = [rnd.choice((0, 1, B28 - 1, rnd.randrange(B28))) for _ in range(13)]
        low = sum(v << (28 * k) for k, v in enumerate(l))
        tmin, tmax = -((low - lo) >> 364), (hi - low) >> 364
        if tmin <= tmax:
            return low + (rnd.randint(tmin, tmax) << 364)


# ------------------------------------------------------------ splitting a sum into terms
def fit(v, sc, xs, lo, hi, rnd, fixed):
    """xs moved inside [lo, hi] until sum sc_i xs_i = v (sc: signed coefficients), or None.
    fixed: {i: value} terms that keep their value"""
    xs = list(xs)
    free = [i for i in range(len(sc)) if i not in fixed and sc[i] != 0]
    rnd.shuffle(free)
    free.sort(key=lambda i: abs(sc[i]) == 1)  # a unit coefficient last: it takes the remainder
    r = v - sum(c * x for c, x in zip(sc, xs))
    for _ in range(2):
        for i in free:
            if r == 0:
                break
            new = min(hi, max(lo, xs[i] + r // sc[i]))
            r -= sc[i] * (new - xs[i])
            xs[i] = new
    return xs if r == 0 else None


def split(v, n, lo, hi, rnd, signs, cmax=7, fixed=None, edgy=False):
    """n (coefficient, value) terms with signed coefficients (magnitude 1..cmax, the sign of term
    i is signs[i]) and values in [lo, hi] that sum to v.  fixed: {i: value} pinned values"""
    fixed = fixed or {}
    xs = [(edgy_value(rnd, lo, hi) if edgy and rnd.random() < 0.3 else rnd.randint(lo, hi)) for _ in range(n)]
    for i, x in fixed.items():
        xs[i] = x
    free = [i for i in range(n) if i not in fixed]
    for attempt in range(200):
        mag = [rnd.randint(1, cmax) for _ in range(n)]
        if attempt >= 8:  # a sum near the end of the range needs the large coefficients
            mag = [cmax] * n
        mag[rnd.choice(free)] = 1
        for i in fixed:  # the pinned values stay light, so the free terms can balance them
            mag[i] = rnd.randint(1, 2)
        sc = [m * s for m, s in zip(mag, signs)]
        pin = sum(sc[i] * fixed[i] for i in fixed)
        top = pin + sum(sc[i] * (hi if sc[i] > 0 else lo) for i in free)
        bot = pin + sum(sc[i] * (lo if sc[i] > 0 else hi) for i in free)
        if not bot <= v <= top:
            continue
        got = fit(v, sc, xs, lo, hi, rnd, fixed)
        if got is not None:
            return list(zip(sc, got))
    raise AssertionError("split: no representation of the sum")


# ============================================================ rp_mul
def _u_columns(x, y):
    """the 64-bit columns of U = x y + m p as the model (and the device) accumulates them"""
    y = y[:14] + [0, 0]
    lo, hi = [0] * 16, [0] * 16
    for i in range(14):
        lo = [a + x[i] * b for a, b in zip(lo, R._shr(y, i))]
    t = R.norm(lo, False)
    t = [t[k] if k < 14 else 0 for k in range(16)]
    mc = [0] * 16
    for i in range(14):
        mc = [a + R.PPL[i] * b for a, b in zip(mc, R._shr(t, i))]
    m = R.norm(mc, False)
    m = [m[k] if k < 14 else 0 for k in range(16)]
    for i in range(14):
        lo = [a + R.PL[i] * b for a, b in zip(lo, R._shr(m, i))]
    return lo


def mont_m(x, y):
    """the Montgomery factor of the product: (x y mod 2^392)(-p^-1) mod 2^392"""
    return R.val(x) * R.val(y) * R.PINV % RP


def _mont_pair(m, rnd, xbound, ybound):
    """x odd with edge limbs and y = -m p x^-1 (mod 2^392) inside (-ybound, ybound)"""
    while True:
        x = edge_slot(rnd, xbound, odd=True)
        y0 = -m * P * pow(R.val(x) % RP, -1, RP) % RP
        if y0 >= RP // 2:
            y0 -= RP
        if abs(y0) < ybound:
            return x, R.limbs(y0)


def rp_mul_records(seed=101):
    rnd = random.Random(seed)
    out = []

    def add(cls, x, y, **kw):
        out.append(Rec(cls, limb_words(x) + limb_words(y), x=list(x), y=list(y), **kw))

    for sx in (1, -1):
        for sy in (1, -1):
            for _ in range(60):
                add("edge_limbs_2p", edge_slot(rnd, 2 * P, sx), edge_slot(rnd, 2 * P, sy))
            for _ in range(60):
                add("edge_limbs_32p", edge_slot(rnd, 32 * P, sx), edge_slot(rnd, 32 * P, sy))
            for _ in range(10):  # no random limb at all
                add("edge_limbs_only", edge_slot(rnd, 2 * P, sx, 0.0), edge_slot(rnd, 32 * P, sy, 0.0))
    for _ in range(40):
        add("random_2p", R.limbs(rnd.randrange(-2 * P + 1, 2 * P)), R.limbs(rnd.randrange(-2 * P + 1, 2 * P)))
    for b in (2 * P, 32 * P):  # the ends of the operand ranges
        for sx in (1, -1):
            for sy in (1, -1):
                add("range_end", respell(R.limbs(sx * (b - 1)), rnd), respell(R.limbs(sy * (b - 1)), rnd))
    zero = [0] * 16
    for _ in range(8):
        add("zero_x", zero, edge_slot(rnd, 32 * P))
        add("zero_y", edge_slot(rnd, 32 * P), zero)
    add("zero_x", zero, zero)
    canon = [0, 1, P - 1]
    for a in canon:
        for b in canon:
            add("canonical", R.to_row(a), R.to_row(b))
            add("canonical", respell(R.to_row(a), rnd), respell(R.to_row(b), rnd))
    # a chosen Montgomery factor m
    alt = sum((M28 if k & 1 else 0) << (28 * k) for k in range(14))
    ms = [("m_one", 1), ("m_all_ones", RP - 1), ("m_alternating", alt), ("m_alternating", (RP - 1) ^ alt)]
    ms += [("m_random", rnd.randrange(RP)) for _ in range(24)]
    for cls, m in ms:
        for xb, yb in ((2 * P, 32 * P), (32 * P, 32 * P)):
            x, y = _mont_pair(m, rnd, xb, yb)
            add(cls, x, y, m=m)
            add(cls, y, x, m=m)
    # x y = 0 (mod 2^392) through powers of two: m = 0
    for s in list(range(8, 385, 8)) + [9, 27, 28, 29, 363, 364, 365, 383]:
        bx = min(2 * P, 32 * P) >> s
        a = rnd.randrange(1, max(bx, 2)) | 1
        b = rnd.randrange(1, max((32 * P) >> (392 - s), 2)) | 1
        if abs(a << s) >= 32 * P or abs(b << (392 - s)) >= 32 * P:
            continue
        sg = rnd.choice((1, -1))
        add("m_zero_pow2", respell(R.limbs(sg * (a << s)), rnd), respell(R.limbs(b << (392 - s)), rnd), m=0)
    # columns: x = (2^28 - T) T^j is 0 spelled in limbs (2^28, -1): the columns of x y cancel,
    # and with y's limbs 10.. zero the columns 11..13 of x y are 0 while 0..10 are large
    for j in range(0, 3):
        for _ in range(6):
            x = [0] * 16
            x[j], x[j + 1] = B28, -1
            y = [rnd.randrange(B28) for _ in range(10 - j)] + [0] * (6 + j)
            add("columns_low_cancel", x, y)
            add("columns_low_cancel", y, x)
    # (the columns 11..13 of U itself are zero only when all of 0..13 are: a non-zero low half makes
    # m non-zero, and m p fills them.)  The reverse holds for U too: x in limbs 11..13 only, y in
    # limbs 0..2 only: columns 0..10 of x y, then of m and of U, are zero and 11..13 are large
    for _ in range(12):
        x = [0] * 11 + [rnd.choice(EDGE[2:]), rnd.randrange(B28), rnd.randrange(-2 * (P >> 364), 2 * (P >> 364)), 0, 0]
        y = [rnd.randrange(1, B28), rnd.choice((0, 1, B28 - 1)), rnd.choice((0, 1)), ] + [0] * 13
        add("columns_top_only", x, y)
        add("columns_top_only", y, x)
    # the low half exactly C 2^392 with no fraction to round: column 13 alone, a multiple of 2^28
    for t in (1, -1, 2 * (P >> 364) - 1, -(2 * (P >> 364)), 16 * (P >> 364)):
        x = [0] * 13 + [t, 0, 0]
        add("low_half_exact", x, [B28] + [0] * 15)
        add("low_half_exact", [B28] + [0] * 15, x)
        add("low_half_exact", [0] * 12 + [B28, t, 0, 0], [0, B28] + [0] * 14)
    return out


def r1_records(seed=102):
    """r1_mul takes both operands distributed; r1_sqr one"""
    src = rp_mul_records(seed)
    keep = [r for i, r in enumerate(src) if i % 3 == 0 or r.cls.startswith(("m_", "col", "canon", "zero", "range"))]
    mul = [Rec(r.cls, r.words, x=r.x, y=r.y) for r in keep]
    sqr = [Rec(r.cls, limb_words(v), x=v, y=v) for r in keep for v in (r.x, r.y)]
    return mul, sqr[:MAX_RECORDS]


# ============================================================ row sums
def _slot_terms(v, n, rnd, cmax=7, edgy=True):
    signs = [rnd.choice((1, -1)) for _ in range(n)]
    if abs(v) > (n - 1) * cmax * P:  # far out: every term pulls the same way
        signs = [1 if v > 0 else -1] * n
    terms = split(v, n, -(2 * P - 1), 2 * P - 1, rnd, signs, cmax, edgy=edgy)
    return [(c, respell(R.limbs(x), rnd, 0.7)) for c, x in terms]


def _acc(terms):
    acc = [0] * 16
    for c, l in terms:
        acc = [a + c * x for a, x in zip(acc, l)]
    return acc


def r_reduce_records(seed=103):
    rnd = random.Random(seed)
    out = []

    def add(cls, terms, **kw):
        acc = _acc(terms)
        assert kw.pop("raw", False) or all(abs(R.val(l)) < 2 * P for _, l in terms)
        acc = acc[:14] + list(kw.pop("lanes", (0, 0)))
        words = [w for a in acc for w in i64_words(a)]
        out.append(Rec(cls, words, terms=terms, acc=acc, v=sum(c * R.val(l) for c, l in terms), **kw))

    ks = sorted(set(list(range(-12, 13)) + list(range(-300, -293)) + list(range(294, 301))
                    + [rnd.randrange(-293, 294) for _ in range(30)]))
    for k in ks:
        for d in DS:
            v = k * P + d
            need = max(1, -(-abs(v) // (7 * (2 * P - 1))) + 1)
            for n in {min(24, need + rnd.randint(0, 3)), min(24, need + rnd.randint(4, 20))}:
                add("kp_plus_d", _slot_terms(v, n, rnd), k=k, d=d)
    for k in (0, 1, -1, 2, -2):  # one term: the value itself
        for d in DS:
            v = k * P + d
            if abs(v) < 2 * P:
                add("one_term", [(1, respell(R.limbs(v), rnd))], k=k, d=d)
                add("one_term", [(-1, respell(R.limbs(-v), rnd))], k=k, d=d)
    for sg in (1, -1):  # 24 terms, every limb sum at its bound
        top = [B28 + 1] * 13
        t = (2 * P - 1 - sum(x << (28 * i) for i, x in enumerate(top))) >> 364
        add("limb_sums_at_bound", [(7 * sg, top + [t, 0, 0])] * 24)
        add("limb_sums_at_bound", [(7 * sg, R.limbs(2 * P - 1))] * 24)
        add("limb_sums_at_bound", [(-7 * sg, [-1] * 13 + [-2 * (P >> 364), 0, 0])] * 24)
        add("limb_sums_at_bound", [(7 * sg, R.limbs(-(2 * P - 1)))] * 24)
    for _ in range(40):  # the top two limb sums zero, the lower ones at their maximum
        n = rnd.randint(1, 24)
        add("top_limbs_zero", [(rnd.choice((7, -7, rnd.randint(-7, 7))), [rnd.choice((B28 + 1, B28 - 1, -1))] * 12 + [0] * 4)
                               for _ in range(n)])
    for _ in range(300):
        n = rnd.randint(1, 24)
        add("edge_limb_terms", [(rnd.choice([c for c in range(-7, 8) if c]), edge_slot(rnd, 2 * P)) for _ in range(n)])
    # the estimate at its limit: the sum already carried (as the staged import's), its low twelve
    # limbs zero, so the top two limbs are v / 2^336 exactly and v is the multiple of 2^336 next
    # above or below k p
    for k in range(-300, 301):
        d = -k * P % (1 << 336)
        for v in (k * P + d, k * P + d - (1 << 336)):
            add("next_to_kp_top_limbs_exact", [(1, R.limbs(v))], raw=True, k=k, d=v - k * P)
    for _ in range(24):  # lanes 14, 15 hold something: the result's are 0 all the same
        n = rnd.randint(1, 24)
        add("lanes_14_15_set", [(rnd.choice([c for c in range(-7, 8) if c]), edge_slot(rnd, 2 * P)) for _ in range(n)],
            lanes=(rnd.choice((1, -1, B28, rnd.randrange(-1 << 40, 1 << 40))), rnd.choice((0, 1, -B28, rnd.randrange(1 << 40)))))
    for n in (24, 36):  # exactly the most terms (36: the Fp12 product's outputs)
        for _ in range(20):
            add("max_terms", [(rnd.choice([c for c in range(-7, 8) if c]), edge_slot(rnd, 2 * P)) for _ in range(n)])
    assert len(out) <= MAX_RECORDS
    return out


def r_operand_records(red, seed=104):
    """up to 8 (slot, coefficient) terms; carry-only sums keep the coefficient sum <= 16"""
    rnd = random.Random(seed + (1 if red else 0))
    out = []

    def add(cls, terms, **kw):
        n = len(terms)
        perm = list(range(8))
        rnd.shuffle(perm)
        slots = [edge_slot(rnd, 2 * P) for _ in range(8)]  # the slots no term reads hold values too
        pairs = []
        for i in range(8):
            c = terms[i][0] if i < n else rnd.choice((5, -3, 7))  # pairs past n: never read
            pairs.append(perm[i] | ((c & 0xFFFF) << 16))
            if i < n:
                slots[perm[i]] = terms[i][1]
        words = [n] + pairs + [w for s in slots for w in limb_words(s)]
        out.append(Rec(cls, words, terms=terms, v=sum(c * R.val(l) for c, l in terms), **kw))

    def coefs(n):
        cm = 7 if red else min(7, 16 // n)
        return [rnd.choice((1, -1)) * rnd.randint(1, cm) for _ in range(n)]

    kmax = 96 if red else 28
    ks = sorted(set(list(range(-6, 7)) + [kmax, -kmax, kmax - 1, 1 - kmax] + [rnd.randrange(-kmax, kmax + 1) for _ in range(12)]))
    for k in ks:
        for d in DS:
            v = k * P + d
            cm = 7 if red else 2
            need = max(1, -(-abs(v) // (cm * (2 * P - 1))) + 1)
            n = min(8, need + rnd.randint(0, 3))
            add("kp_plus_d", _slot_terms(v, n, rnd, cm), k=k, d=d)
    for n in range(1, 9):
        for _ in range(25):
            add("edge_limb_terms_n%d" % n, list(zip(coefs(n), [edge_slot(rnd, 2 * P) for _ in range(n)])))
    for sg in (1, -1):
        c = 7 if red else 2
        add("limb_sums_at_bound", [(c * sg, [B28 + 1] * 13 + [2 * (P >> 364) - 2, 0, 0])] * 8)
        add("limb_sums_at_bound", [(c * sg, [-1] * 13 + [-2 * (P >> 364), 0, 0])] * 8)
    if red:
        for _ in range(10):
            add("coefficient_12", [(rnd.choice((12, -12)), edge_slot(rnd, 2 * P)) for _ in range(rnd.randint(1, 8))])
    return out


def rfp_records(seed=105):
    """a, b: rfp values (slot range) for f_add, f_sub, f_neg, f_mul3, f_mul8, f_mul"""
    rnd = random.Random(seed)
    out = []

    def add(cls, a, b):
        out.append(Rec(cls, limb_words(a) + limb_words(b), x=list(a), y=list(b)))

    for _ in range(150):
        add("edge_limbs_2p", edge_slot(rnd, 2 * P), edge_slot(rnd, 2 * P))
    for k in (-2, -1, 0, 1):  # a + b, a - b, 3 a, 8 a next to multiples of p
        for d in DS:
            for t in (1, 2, 3, 8):
                # a with t a = k' p + d for some k'
                kk = rnd.randrange(-2 * t + 1, 2 * t)
                if (kk * P + d) % t:
                    continue
                a = (kk * P + d) // t
                if abs(a) >= 2 * P:
                    continue
                b = rnd.choice((k * P + d - a, a - (k * P + d)))
                if abs(b) >= 2 * P:
                    b = rnd.randrange(-2 * P + 1, 2 * P)
                add("near_multiple_of_p", respell(R.limbs(a), rnd), respell(R.limbs(b), rnd))
    for a in (0, 1, P - 1):
        for b in (0, 1, P - 1):
            add("canonical", R.to_row(a), respell(R.to_row(b), rnd))
    for sa in (1, -1):
        for sb in (1, -1):
            add("range_end", R.limbs(sa * (2 * P - 1)), R.limbs(sb * (2 * P - 1)))
    return out


# ============================================================ canonical forms, import / export
def canon_records(seed=106):
    """representatives of one residue across (-2p, 2p), in several limb spellings"""
    rnd = random.Random(seed)
    out = []

    def add(cls, l):
        out.append(Rec(cls, limb_words(l), x=list(l), v=R.val(l)))

    res = [("residue_0", 0), ("residue_1", 1), ("residue_p_minus_1", P - 1)]
    res += [("residue_random", rnd.randrange(P)) for _ in range(12)]
    res += [("residue_edgy", edgy_value(rnd, 0, P - 1)) for _ in range(12)]
    for cls, a in res:
        for j in (-2, -1, 0, 1, 2):
            v = a + j * P
            if abs(v) >= 2 * P:
                continue
            add(cls, R.limbs(v))
            for _ in range(3):
                add(cls, respell(R.limbs(v), rnd, 0.9))
    for _ in range(120):
        add("edge_limbs", edge_slot(rnd, 2 * P))
    for v in (2 * P - 1, -(2 * P - 1)):
        add("range_end", R.limbs(v))
        add("range_end", respell(R.limbs(v), rnd, 0.9))
    return out


def import_records(seed=107):
    """canonical fp values (2^384-Montgomery words) through import and export"""
    rnd = random.Random(seed)
    out = []
    vals = [("value_0", 0), ("value_1", 1), ("value_p_minus_1", P - 1), ("value_top", (P - 1) >> 8 << 8)]
    vals += [("value_random", rnd.randrange(P)) for _ in range(60)]
    vals += [("value_edgy", edgy_value(rnd, 0, P - 1)) for _ in range(40)]
    # a 2^8 next to a multiple of p: the import's quotient estimate at its limits
    for k in range(0, 256, 5):
        for d in (0, 1, 2, 255, 256, 257):
            a = -(-(k * P + d) // 256)
            if a < P:
                vals.append(("near_multiple_of_p", a))
    for cls, a in vals:
        out.append(Rec(cls, fp_words(a), a=a))
    return out


# ============================================================ wave / group reductions
def w_lin_records(maxn, seed=108):
    """np added and nn subtracted terms, values in [0, 3p), coefficients 0..7"""
    rnd = random.Random(seed + maxn)
    out = []
    hi = 3 * P - 1

    def add(cls, pa, na, **kw):
        np_, nn = len(pa), len(na)
        assert np_ + nn <= maxn
        terms = [None] * maxn
        for i, t in enumerate(pa):
            terms[i] = t
        for i, t in enumerate(na):
            terms[maxn - nn + i] = t
        words = [np_, nn]
        for t in terms:
            c, x = t if t is not None else (5, rnd.randrange(3 * P))  # padding: a value, a coefficient
            words += fp_words(x) + [c]
        v = sum(c * x for c, x in pa) - sum(c * x for c, x in na)
        out.append(Rec(cls, words, pa=list(pa), na=list(na), v=v, **kw))

    def terms_for(v, np_, nn, fixed=None):
        signs = [1] * np_ + [-1] * nn
        t = split(v, np_ + nn, 0, hi, rnd, signs, 7, fixed, edgy=True)
        return [(c, x) for c, x in t[:np_]], [(-c, x) for c, x in t[np_:]]

    kmax = 21 * maxn - 20  # 7 * 3 * maxn less the term that takes the remainder
    ks = sorted(set(list(range(-8, 9)) + list(range(-kmax, -kmax + 4)) + list(range(kmax - 3, kmax + 1))
                    + [rnd.randrange(-kmax, kmax + 1) for _ in range(20)]))
    for k in ks:
        for d in DS:
            v = k * P + d
            need = max(1, -(-abs(v) // (7 * hi)) + 1)
            for rep in range(2):
                if v >= 0:
                    np_ = min(maxn, need + rnd.randint(0, 3))
                    nn = rnd.randint(0, min(maxn - np_, 4 if rep else maxn))
                else:
                    nn = min(maxn, need + rnd.randint(0, 3))
                    np_ = rnd.randint(0, min(maxn - nn, 4 if rep else maxn))
                if abs(v) < 7 * hi and rep:  # any sign split, every slot used
                    np_ = rnd.randint(1, maxn - 1)
                    nn = maxn - np_
                pa, na = terms_for(v, np_, nn)
                add("kp_plus_d", pa, na, k=k, d=d)
    # the estimate at its limit: every value a multiple of 2^320, so limbs 10 and 11 give
    # V / 2^320 exactly, and V is the multiple of 2^320 next above or below k p
    for k in range(-kmax + 2, kmax - 1, 4):
        d = -k * P % (1 << 320)
        for v in (k * P + d, k * P + d - (1 << 320)):
            need = max(1, -(-abs(v) // (7 * hi)) + 2)
            big, small = min(maxn, need + rnd.randint(0, 3)), rnd.randint(0, 3)
            small = min(small, maxn - big)
            np_, nn = (big, small) if v >= 0 else (small, big)
            t = split(v >> 320, np_ + nn, 0, hi >> 320, rnd, [1] * np_ + [-1] * nn, 7)
            add("next_to_kp_top_limbs_exact", [(c, x << 320) for c, x in t[:np_]], [(-c, x << 320) for c, x in t[np_:]],
                k=k, d=v - k * P)
    for d in DS:  # one sign only
        for k in (0, 1, 2, 5, 40):
            n = rnd.randint(min(maxn, (k + 1) // 21 + 2), maxn)
            if k * P + d >= 0:
                pa, na = terms_for(k * P + d, n, 0)
                add("nn_zero", pa, na, k=k, d=d)
            if -k * P + d <= 0:
                pa, na = terms_for(-k * P + d, 0, n)
                add("np_zero", pa, na, k=-k, d=d)
    for d in DS:  # exactly MAXN terms
        for k in (-3, 0, 3, kmax // 2):
            np_ = rnd.randint(1, maxn - 1) if k < kmax // 2 else maxn
            pa, na = terms_for(k * P + d, np_, maxn - np_)
            add("max_terms", pa, na, k=k, d=d)
    for x in (0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, hi):  # one term
        add("one_term", [(1, x)], [])
        add("one_term", [], [(1, x)])
        add("one_term", [(7, x)], [])
        add("one_term", [(0, x)], [])
    for k in range(-4, 5):  # the values 0, p, 2p, 3p - 1 among the terms
        for d in DS[:5]:
            n = maxn
            fixed = {0: 0, 1: P, n - 2: 2 * P, n - 1: hi}
            np_ = rnd.randint(4, n - 4)
            pa, na = terms_for(k * P + d, np_, n - np_, fixed)
            add("special_values", pa, na, k=k, d=d)
    ones = (1 << 352) - 1
    xmax = ((hi >> 352) << 352) | ones
    xmax = xmax if xmax <= hi else xmax - (1 << 352)
    for n in (1, maxn // 2, maxn):  # every limb sum at its bound
        add("limb_sums_at_bound", [(7, xmax)] * n, [])
        add("limb_sums_at_bound", [], [(7, xmax)] * n)
        add("limb_sums_at_bound", [(7, hi)] * n, [])
        add("limb_sums_at_bound", [], [(7, hi)] * n)
        add("limb_sums_at_bound", [(7, xmax)] * (n // 2), [(7, ones)] * (maxn - n // 2))
    low = (1 << 320) - 1
    for n in range(1, maxn + 1):  # limbs 10 and 11 zero, the lower ones at their maximum
        add("top_limbs_zero", [(7, low)] * n, [])
        add("top_limbs_zero", [], [(7, low)] * n)
        k = rnd.randint(0, n)
        add("top_limbs_zero", [(rnd.randint(0, 7), low)] * k, [(rnd.randint(1, 7), low)] * (n - k))
    for _ in range(200):
        n = rnd.randint(1, maxn)
        t = [(rnd.randint(0, 7), rnd.choice([rnd.randrange(3 * P), hi, 0, P, edgy_value(rnd, 0, hi)])) for _ in range(n)]
        k = rnd.randint(0, n)
        add("random_terms", t[:k], t[k:])
    assert len(out) <= MAX_RECORDS
    return out


def g_reduce_records(src):
    """the 64-bit limb sums of the w_lin<MAXL> terms (src: w_lin_records(MAXL))"""
    out = []
    for r in src:
        def sums(ts):
            return [sum(c * ((x >> (32 * j)) & 0xFFFFFFFF) for c, x in ts) for j in range(12)]
        pa, na = sums(r.pa), sums(r.na)
        words = [w for s in pa + na for w in (s & 0xFFFFFFFF, s >> 32)]
        out.append(Rec(r.cls, words, **{k: v for k, v in r.__dict__.items() if k not in ("cls", "words")}))
    return out


# ============================================================ Fp12 level
def _o():
    from oracle import bls_oracle as o
    return o


def f12_flat(a):
    return [c for h in a for x in h for c in x]


def f12_tower(v):
    return tuple(tuple((v[6 * h + 2 * j], v[6 * h + 2 * j + 1]) for j in range(3)) for h in range(2))


def f12_words(v):
    return [w for c in v for w in fp_words(mont(c))]


def f12_of_words(words):
    return [unmont(fp_of_words(words[12 * k:12 * k + 12])) for k in range(12)]


_F12 = None


def f12_elements():
    """(class, 12 coefficients) in slot order"""
    global _F12
    if _F12 is not None:
        return _F12
    o = _o()
    rnd = random.Random(110)
    els = [("zero", [0] * 12), ("one", [1] + [0] * 11), ("minus_one", [P - 1] + [0] * 11), ("all_p_minus_1", [P - 1] * 12)]
    for k in range(12):
        els.append(("unit_%d" % k, [rnd.randrange(1, P) if j == k else 0 for j in range(12)]))
    for _ in range(2):  # a line's shape: c0.c0, c0.c1 and c1.c1 only
        els.append(("sparse_line", [rnd.randrange(P) if j in (0, 1, 2, 3, 8, 9) else 0 for j in range(12)]))
    for i in range(2):  # f^((p^6 - 1)(p^2 + 1)) of a Miller value
        f = o.miller_loop(o.G1, o.hash_to_g2(bytes([i + 1]) * 32))
        g = o.f12_mul(o.f12_conj(f), o.f12_inv(f))
        g = o.f12_mul(o.f12_pow(g, P * P), g)
        els.append(("cyclotomic", f12_flat(g)))
    for _ in range(3):
        els.append(("random", [rnd.randrange(P) for _ in range(12)]))
    _F12 = els
    return els


def f12_records():
    """op -> records for the Fp12-level operations of both engines"""
    els = f12_elements()
    rnd = random.Random(111)
    rec = {}
    unary = [Rec(c, f12_words(a), a=a) for c, a in els]
    frob_cls = ("zero", "one", "all_p_minus_1", "unit_3", "unit_10", "sparse_line", "cyclotomic", "random")
    rec["sqr"] = unary
    rec["frob"] = [r for r in unary if r.cls in frob_cls]
    rec["frob2"] = rec["frob"]
    rec["conj"] = unary
    rec["inv"] = [r for r in unary if r.cls != "zero"]
    rec["csqr"] = [r for r in unary if r.cls in ("cyclotomic", "one")]
    rec["mul"] = []
    rnds = [a for c, a in els if c == "random"]
    for i, (c, a) in enumerate(els):
        for b in (rnds[i % len(rnds)], els[(i + 5) % len(els)][1], a):
            rec["mul"].append(Rec(c, f12_words(a) + f12_words(b), a=a, b=b))
    rec["is_one"] = unary + [Rec("one_plus_last", f12_words([1] + [0] * 10 + [1]), a=[1] + [0] * 10 + [1]),
                             Rec("p_minus_1_first", f12_words([P - 1] + [0] * 11), a=[P - 1] + [0] * 11)]
    rec["eq"] = []
    for c, a in els:
        rec["eq"].append(Rec(c + "_same", f12_words(a) + f12_words(a), a=a, b=a))
        k = rnd.randrange(12)
        b = [(x + 1) % P if j == k else x for j, x in enumerate(a)]
        rec["eq"].append(Rec(c + "_one_off", f12_words(a) + f12_words(b), a=a, b=b))
    return rec


def pdbl_records(seed=112):
    """a random projective representation of a hashed point, doubled k times in a row"""
    o = _o()
    rnd = random.Random(seed)
    out = []
    for i, chain in enumerate((1, 2, PDBL_CHAIN)):
        A = o.hash_to_g2(bytes([i, 9]) * 16)
        z = (rnd.randrange(1, P), rnd.randrange(P))
        pt = [c for v in (o.f2_mul(A[0], z), o.f2_mul(A[1], z), z) for c in v]
        words = [chain] + [w for c in pt for w in fp_words(mont(c))]
        out.append(Rec("chain_%d" % chain, words, point=A, chain=chain))
    return out


# ============================================================ the whole set
_ALL = None


def all_records():
    """op name (as in OPS) -> records"""
    global _ALL
    if _ALL is not None:
        return _ALL
    recs = {}
    recs["rp_mul"] = rp_mul_records()
    recs["r1_mul"], recs["r1_sqr"] = r1_records()
    recs["r_reduce"] = r_reduce_records()
    rf = rfp_records()
    for name in ("f_add", "f_sub", "f_neg", "f_mul3", "f_mul8", "f_mul"):
        recs[name] = rf
    recs["r_operand_carry"] = r_operand_records(False)
    recs["r_operand_red"] = r_operand_records(True)
    cn = canon_records()
    recs["r_canon"] = recs["r_export"] = recs["r1_export"] = cn
    recs["r_import_export"] = recs["r1_import_export"] = import_records()
    recs["w_lin_maxp"] = recs["w_lin_maxp_full"] = w_lin_records(MAXP)
    recs["w_lin_maxl"] = recs["w_lin_maxl_full"] = w_lin_records(MAXL)
    recs["g_reduce"] = recs["g_reduce_full"] = g_reduce_records(recs["w_lin_maxl"])
    f12 = f12_records()
    for eng in "rw":
        for op in ("mul", "sqr", "frob", "frob2", "is_one"):
            recs[eng + "_" + op] = f12[op]
    recs["r_csqr"], recs["r_eq"] = f12["csqr"], f12["eq"]
    recs["w_conj"], recs["w_inv"] = f12["conj"], f12["inv"]
    recs["r_pdbl_fast"] = pdbl_records()
    for name, rs in recs.items():
        assert 0 < len(rs) <= MAX_RECORDS, name
        for r in rs:
            assert len(r.words) == OPS[name][1], (name, r.cls, len(r.words))
    _ALL = recs
    return recs


def class_counts(recs=None):
    recs = recs or all_records()
    out = {}
    for name, rs in recs.items():
        c = {}
        for r in rs:
            c[r.cls] = c.get(r.cls, 0) + 1
        out[name] = c
    return out


def pack_input(recs=None):
    """the carrier's input file"""
    recs = recs or all_records()
    parts = [struct.pack("<II", MAGIC, len(recs))]
    for name, rs in recs.items():
        op, iw, ow = OPS[name]
        words = [u32(w) for r in rs for w in r.words]
        parts.append(struct.pack("<IIII", op, len(rs), iw, ow))
        parts.append(struct.pack("<%dI" % len(words), *words))
    return b"".join(parts)


def parse_output(data, recs=None):
    """op name -> one list of output words per record"""
    recs = recs or all_records()
    total = sum(len(rs) * OPS[name][2] for name, rs in recs.items())
    assert len(data) == 4 * total, "output size %d, expected %d" % (len(data), 4 * total)
    words = struct.unpack("<%dI" % total, data)
    out, pos = {}, 0
    for name, rs in recs.items():
        ow = OPS[name][2]
        out[name] = [list(words[pos + i * ow: pos + (i + 1) * ow]) for i in range(len(rs))]
        pos += len(rs) * ow
    return out


# ============================================================ the exact conditions and the models
# Every function returns None, or what is wrong as a string; `r` is a result as the carrier wrote
# it (the tests pass the model's result through the same functions).
LIMB_LO, LIMB_HI = -1, B28 + 2  # limbs 0..12 of a row value lie in [LIMB_LO, LIMB_HI)


def _row_shape(r):
    if len(r) != 16 or r[14] != 0 or r[15] != 0:
        return "lanes 14, 15 not zero: %r" % (r[14:],)
    bad = [(k, x) for k, x in enumerate(r[:13]) if not LIMB_LO <= x < LIMB_HI]
    if bad:
        return "limbs outside [%d, 2^28 + %d): %r" % (LIMB_LO, LIMB_HI - B28, bad)
    return None


def exact_row_product(x, y, r):
    """r = x y / 2^392 (mod p), |r| < |x y| / 2^392 + 1.0001 p, limbs in range"""
    e = _row_shape(r)
    if e:
        return e
    xy, v = R.val(x) * R.val(y), R.val(r)
    if (v * RP - xy) % P:
        return "not congruent to x y / 2^392"
    if abs(v) * RP * 10000 >= abs(xy) * 10000 + 10001 * P * RP:
        return "|r| >= |x y| / 2^392 + 1.0001 p"
    return None


def exact_row_sum(v, r, reduced):
    """reduced: r = v (mod p) within [-p / 2^20, p + p / 2^20); carries only: r = v"""
    e = _row_shape(r)
    if e:
        return e
    got = R.val(r)
    if not reduced:
        return None if got == v else "value changed by the carries: off by %d" % (got - v)
    if (got - v) % P:
        return "not congruent to the sum"
    if not -(P >> 20) <= got < P + (P >> 20):
        return "outside [-p / 2^20, p + p / 2^20): r / p = %.9f" % (got / P)
    return None


def exact_wave_sum(v, words, full):
    """[0, 3p) and congruent; below p when full"""
    got = fp_of_words(words)
    if (got - v) % P:
        return "not congruent to the sum"
    if not 0 <= got < (P if full else 3 * P):
        return "outside [0, %s): r / p = %.6f" % ("p" if full else "3p", got / P)
    return None


def model_wave_sum(rec, full):
    r = rec.v - (G.quotient_estimate(rec.pa, rec.na) - 1) * P
    return r % P if full else r


RFP_TERMS = {"f_add": (1, 1), "f_sub": (1, -1), "f_neg": (-1, 0), "f_mul3": (3, 0), "f_mul8": (8, 0)}


def rfp_terms(name, rec):
    ca, cb = RFP_TERMS[name]
    return [(ca, rec.x)] + ([(cb, rec.y)] if cb else [])


def export_expected(v):
    """canonical words of a row value taken from R' = 2^392 to the 2^384-Montgomery form"""
    return fp_words(v * pow(256, -1, P) % P)
