"""tests/golden/miller28_pairs.txt: (P, Q) pairs for the host check of the limb-resident per-root
Miller loop (tests/native/miller28_check.cpp), from the CPU oracle's arithmetic.  One pair per line:
  <kind> <P.x> <P.y> <Q.x.c0> <Q.x.c1> <Q.y.c0> <Q.y.c1>      (plain integers, 96 hex digits each)
kinds: rand (P in G1, Q in G2), gen (both generators), zero_x (P = (0, 2) or (0, -2): a curve point
with a zero coordinate, all-zero limbs in the line products), pm1 (a coordinate of P equal to p - 1).
The check compares two evaluations of the same polynomial map in P's and Q's coordinates, so it needs
no subgroup membership: (0, 2) has order 3, and the pm1 points lie off the curve where the curve has
no such point (x = p - 1 needs y^2 = 3, a non-residue; y = p - 1 needs a cube root of -3, which is no cube).

  python tools/gen_miller28_vectors.py > tests/golden/miller28_pairs.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.bls_oracle as o  # noqa: E402

G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


def g2_point(seed):
    return o.hash_to_g2(bytes([seed]) * 32)


def pm1_points():
    """P with a coordinate equal to p - 1; the curve has no such point (see above), so off it"""
    return [(o.P - 1, 5), (7, o.P - 1)]


def main():
    assert o.g2_on_curve(G2) and o.g2_in_subgroup_slow(G2)
    rows = []
    for s in range(6):
        P = o.g1_mul(o.G1, 0x9E3779B97F4A7C15 * (s + 1) + s)
        Q = g2_point(s)
        assert o.g1_on_curve(P) and o.g2_in_subgroup_slow(Q)
        rows.append(("rand", P, Q))
    rows.append(("gen", o.G1, G2))
    rows.append(("gen", o.G1, g2_point(0x40)))
    assert o.g1_on_curve((0, 2))
    rows.append(("zero_x", (0, 2), G2))
    rows.append(("zero_x", (0, o.P - 2), g2_point(0x41)))
    for i, P in enumerate(pm1_points()):
        rows.append(("pm1", P, g2_point(0x42 + i)))
    for kind, P, Q in rows:
        (x0, x1), (y0, y1) = Q
        print(kind, *("%096x" % v for v in (P[0], P[1], x0, x1, y0, y1)))


if __name__ == "__main__":
    main()
