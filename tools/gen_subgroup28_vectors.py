"""tests/golden/subgroup28_points.txt: affine points of E'(Fp2) for the limb-resident psi-ladder's
host checks (tests/native/fp2_28_check.cpp), from the CPU oracle.  One point per line:
  <kind> <expected 1|0> <x.c0> <x.c1> <y.c0> <y.c1>      (plain integers, 96 hex digits each)
kinds: g2 (in the subgroup), curve (on the curve, outside G2: a mapped point before the cofactor is
cleared), ord13 / ord23 (the small-order points of tests/test_gpu_parity.py: an order-13 point meets
acc == -P at bit 60, runs on at infinity and restarts from P at bit 57), mixed (a G2 point plus a
small-order one).
The ladder's other exceptional addition, acc == +P, needs a point whose order divides one of
2 - 1, 12 - 1, 104 - 1, 53760 - 1, 53761 2^32 - 1 (the ladder's prefixes before its additions, less
one); none of them shares a factor with the curve's order h2 r (checked below), so no curve point
reaches it: the host check enters that branch through the addition itself (acc = P).

  python tools/gen_subgroup28_vectors.py > tests/golden/subgroup28_points.txt
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.bls_oracle as o  # noqa: E402

H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5


def mapped(seed):
    u = o.hash_to_field_fp2(bytes([seed]) * 32, 2, o.DST_POP)[0]
    return o.iso_map(o.map_to_curve_sswu(u))


def main():
    x = -o.BLS_X
    acc, pre = 1, []
    for b in range(62, -1, -1):
        acc *= 2
        if (x >> b) & 1:
            pre.append(acc)
            acc += 1
    assert acc == x and pre == [2, 12, 104, 53760, 53761 << 32]
    assert all(math.gcd(v - 1, H2 * o.R) == 1 for v in pre), "acc == +P is reachable: add such a point"
    rows = []
    for s in range(6):
        q = mapped(s)
        assert o.g2_on_curve(q) and not o.g2_in_subgroup_slow(q)
        rows.append(("curve", 0, q))
        g = o.g2_clear_cofactor(q)
        assert o.g2_in_subgroup_slow(g)
        rows.append(("g2", 1, g))
    q = mapped(0x20)
    small = []
    for ell in (13, 23):
        Q = o.g2_mul(q, H2 * o.R // (ell * ell))
        if Q is not None and o.g2_mul(Q, ell) is not None:
            Q = o.g2_mul(Q, ell)
        assert Q is not None and o.g2_mul(Q, ell) is None
        small.append(Q)
        rows.append((f"ord{ell}", 0, Q))
        rows.append((f"ord{ell}", 0, o.g2_neg(Q)))
        for k in (2, 5):
            rows.append((f"ord{ell}", 0, o.g2_mul(Q, k)))
    g = o.g2_clear_cofactor(mapped(0x21))
    for Q in small:
        rows.append(("mixed", 0, o.g2_add(g, Q)))
    for kind, exp, pt in rows:
        (x0, x1), (y0, y1) = pt
        print(kind, exp, *("%096x" % v for v in (x0, x1, y0, y1)))


if __name__ == "__main__":
    main()
