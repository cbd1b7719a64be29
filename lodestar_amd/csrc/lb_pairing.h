// Optimal-ate Miller loop and final exponentiation for BLS12-381 (M-type sextic twist,
// y^2 = x^3 + 4(1+u)).  Replaces blst's miller_loop_n / final_exp behind
// Pairing.commit + Pairing.finalverify (maybeBatch.ts:18-25).
//
// Lines are evaluated at the G1 point P = (xP, yP) and kept in the sparse form
//   l = l0 + l2 w^2 + l3 w^3      (Fp12 = Fp6[w]/(w^2 - v))
// which differs from the textbook line value only by factors in Fp4, killed by the
// final exponentiation.  The hard part computes f^(3(p^4-p^2+1)/r); cubing is a
// bijection on the order-r group, so "== 1" decides exactly as blst's finalverify.
#pragma once
#include "lb_curve.h"

// doubling step on T = (X, Y, Z) (homogeneous projective on the twist), line at P.
// 25 Fp multiplications: 3b' = 12(1 + u) is applied with additions, and the output is scaled
// by 4 (a homogeneous (X:Y:Z) ~ (4X:4Y:4Z)) so the textbook halvings of X3, Y3 disappear.
template <bool kInl = false>
LB_HD void miller_dbl(g2j& T, fp2& l0, fp2& l2, fp2& l3, const fp& xP, const fp& yP) {
  fp2 X = T.x, Y = T.y, Z = T.z;
  fp2 A = lean2_mul<kInl>(X, Y);             // XY
  fp2 B = lean2_sqr<kInl>(Y);
  fp2 C = lean2_sqr<kInl>(Z);
  fp2 E = fp2_mul3(fp2_dbl(fp2_dbl(fp2_mul_xi(C))));  // 3b' Z^2 = 12 (1 + u) Z^2
  fp2 F = fp2_mul3(E);               // 9b' Z^2
  fp2 H = fp2_sub(lean2_sqr<kInl>(fp2_add(Y, Z)), fp2_add(B, C));  // 2YZ
  fp2 XX3 = fp2_mul3(lean2_sqr<kInl>(X));
  // line: (B - E) + (-3X^2 xP) w^2 + (H yP) w^3
  l0 = fp2_sub(B, E);
  l2 = fp2_neg(fp2{lean_mul<kInl>(XX3.c0, xP), lean_mul<kInl>(XX3.c1, xP)});
  l3 = fp2{lean_mul<kInl>(H.c0, yP), lean_mul<kInl>(H.c1, yP)};
  // 4 x (X3, Y3, Z3) with X3 = XY/2 (B - F), Y3 = ((B+F)/2)^2 - 3E^2, Z3 = B H:
  //   X3' = 2 A (B - F),  Y3' = (B + F)^2 - 12 E^2,  Z3' = 4 B H
  T.x = fp2_dbl(lean2_mul<kInl>(A, fp2_sub(B, F)));
  T.y = fp2_sub(lean2_sqr<kInl>(fp2_add(B, F)), fp2_mul3(fp2_dbl(fp2_dbl(lean2_sqr<kInl>(E)))));
  T.z = fp2_dbl(fp2_dbl(lean2_mul<kInl>(B, H)));
}

// addition step T <- T + Q (Q affine), line through T and Q at P
template <bool kInl = false>
LB_HD void miller_add(g2j& T, const g2a& Q, fp2& l0, fp2& l2, fp2& l3, const fp& xP, const fp& yP) {
  fp2 theta = fp2_sub(T.y, lean2_mul<kInl>(Q.y, T.z));
  fp2 lam = fp2_sub(T.x, lean2_mul<kInl>(Q.x, T.z));
  // line: (theta xQ - lam yQ) + (-theta xP) w^2 + (lam yP) w^3
  l0 = fp2_sub(lean2_mul<kInl>(theta, Q.x), lean2_mul<kInl>(lam, Q.y));
  l2 = fp2_neg(fp2{lean_mul<kInl>(theta.c0, xP), lean_mul<kInl>(theta.c1, xP)});
  l3 = fp2{lean_mul<kInl>(lam.c0, yP), lean_mul<kInl>(lam.c1, yP)};
  fp2 C = lean2_sqr<kInl>(theta);
  fp2 D = lean2_sqr<kInl>(lam);
  fp2 E = lean2_mul<kInl>(lam, D);
  fp2 F = lean2_mul<kInl>(T.z, C);
  fp2 G = lean2_mul<kInl>(T.x, D);
  fp2 H = fp2_sub(fp2_add(E, F), fp2_dbl(G));
  T.x = lean2_mul<kInl>(lam, H);
  T.y = fp2_sub(lean2_mul<kInl>(theta, fp2_sub(G, H)), lean2_mul<kInl>(E, T.y));
  T.z = lean2_mul<kInl>(T.z, E);
}

// f_{|x|,Q}(P), conjugated (x < 0).  P, Q affine and not infinity.
LB_NI fp12 miller_loop(g1a P, g2a Q) {
  g2j T;
  T.x = Q.x;
  T.y = Q.y;
  T.z = fp2_one();
  fp2 l0, l2, l3;
  fp12 f = fp12_one();
  bool first = true;
  for (int i = 62; i >= 0; i--) {
    if (!first) f = fp12_sqr(f);
    miller_dbl(T, l0, l2, l3, P.x, P.y);
    if (first) {
      f = fp12_one();
      first = false;
    }
    f = fp12_mul_line(f, l0, l2, l3);
    if ((LB_X_ABS >> i) & 1ull) {
      miller_add(T, Q, l0, l2, l3, P.x, P.y);
      f = fp12_mul_line(f, l0, l2, l3);
    }
  }
  return fp12_conj(f);
}

// Same loop with the Fp12 squaring / line multiplication / point steps inlined, so f, T and
// the line values stay in registers (only fp_mul is a call).  The pointer-argument versions
// cost ~8 GB of scratch traffic per 19k-pair launch (profiles/r1_pmc_*).
LB_HD fp12 miller_loop_inl(const g1a& P, const g2a& Q) {
  g2j T;
  T.x = Q.x;
  T.y = Q.y;
  T.z = fp2_one();
  fp2 l0, l2, l3;
  fp12 f = fp12_one();
  bool first = true;
  for (int i = 62; i >= 0; i--) {
    if (!first) f = fp12_sqr_inl(f);
    miller_dbl(T, l0, l2, l3, P.x, P.y);
    if (first) {
      f = fp12_one();
      first = false;
    }
    f = fp12_mul_line_inl(f, l0, l2, l3);
    if ((LB_X_ABS >> i) & 1ull) {
      miller_add(T, Q, l0, l2, l3, P.x, P.y);
      f = fp12_mul_line_inl(f, l0, l2, l3);
    }
  }
  return fp12_conj(f);
}

// ---- The same loop in 28-bit limbs from product to product (lb_field.h: fp2_28, fp6_28), for the
// one-lane-per-root kernel k_miller_lane.  Formulas, statement order and product tree are those of
// miller_dbl / miller_add / fp12_sqr_inl / fp12_mul_line_inl; only the representation between the
// products changes.  The state lives in four slots of 3 fp2_28 each behind S.get2(k, i) /
// S.put2(k, i, v): 0, 1 = f.c0, f.c1; 2 = a tower temporary; 3 = T = (X, Y, Z).
// Loop invariant, at the top of a step and again before its addition pass: every stored
// coefficient has limbs 0..12 below 2^28, and per component, in units of p,
//   f.c0 <= (VF00, VF01, VF02),  f.c1 <= (VF10, VF11, VF12),  X <= VX, Y <= VY, Z <= VZ.
// The bounds differ per coefficient because the subtraction constants do: a coefficient that is a
// product minus two others carries their K.  The comments give each value's bound as in lb_curve.h
// (a product's output is 1 + S / 2520); the LB_FP28_CHECK host build (tests/native/
// miller28_check.cpp) re-assumes exactly this invariant at both places and propagates worst-case
// limb and value bounds through the straight-line step, so one pass proves the step for every
// input: a doubling step, a doubling step followed by an addition pass, and the first step.
#define LB_M28_VF00 10.0
#define LB_M28_VF01 14.0
#define LB_M28_VF02 6.0
#define LB_M28_VF10 20.0
#define LB_M28_VF11 27.0
#define LB_M28_VF12 17.0
#define LB_M28_VX 8.0
#define LB_M28_VY 72.0
#define LB_M28_VZ 8.0
#define LB_M28_CONJ_C 28  // the K of the final conjugation K - f.c1: above every VF1x
#if defined(LB_FP28_CHECK)
static inline void fp2_28_chk_assume(fp2_28& a, double vb) { fp28_chk_assume(a.c0, vb), fp28_chk_assume(a.c1, vb); }
template <class S_t>
static inline void miller28_chk_assume(const S_t& S) {
  const double vf[2][3] = {{LB_M28_VF00, LB_M28_VF01, LB_M28_VF02}, {LB_M28_VF10, LB_M28_VF11, LB_M28_VF12}};
  const double vt[3] = {LB_M28_VX, LB_M28_VY, LB_M28_VZ};
  for (int k = 0; k < 2; k++)
    for (int i = 0; i < 3; i++) {
      fp2_28 v = S.get2(k, i);
      fp2_28_chk_assume(v, vf[k][i]);
      S.put2(k, i, v);
    }
  for (int i = 0; i < 3; i++) {
    fp2_28 v = S.get2(3, i);
    fp2_28_chk_assume(v, vt[i]);
    S.put2(3, i, v);
  }
}
#endif

// doubling step on T = (X, Y, Z) <= (8, 72, 8) p, P's coordinates as the limbs of a 2^8 (256 p: they
// meet 3 X^2 and H in a product at once).  Lines leave normalised: l0 <= 48, l2 <= 2, l3 <= 4.
LB_HD void miller_dbl28(fp2_28& X, fp2_28& Y, fp2_28& Z, fp2_28& l0, fp2_28& l2, fp2_28& l3, const fp28& xP,
                        const fp28& yP) {
  const fp2_28 A = fp2_28_mul<73, 28>(X, Y);                                  // 8 (72 + 73) -> 1.47
  const fp2_28 B = fp2_28_sqr<73, 28>(Y);                                     // 144 x 145 -> 9.29
  const fp2_28 C = fp2_28_sqr<9, 28>(Z);                                      // 16 x 17 -> 1.11
  // 3b' Z^2 = 12 xi C: xi C <= 3.11, limbs 3 x 2^28; x 4 normalised; x 3 normalised: 37.4
  const fp2_28 E = fp2_28_norm(fp2_28_muls<3>(fp2_28_norm(fp2_28_muls<4>(fp2_28_mul_xi<2, 28>(C)))));
  // 2 Y Z = (Y + Z)^2 - (B + C): 160 x 161 -> 11.3; + 11 = 22.3, limbs 4 x 2^28
  const fp2_28 H = fp2_28_sub<11, 29>(fp2_28_sqr<81, 28>(fp2_28_norm(fp2_28_add(Y, Z))), fp2_28_add(B, C));
  const fp2_28 XX3 = fp2_28_muls<3>(fp2_28_sqr<9, 28>(X));                    // 3 x 1.11 = 3.33, limbs 3 x 2^28
  l0 = fp2_28_norm(fp2_28_sub<38, 28>(B, E));                                 // 9.29 + 38 = 47.3
  l2 = fp2_28_norm(fp2_28_kminus<2, 28>(fp2_28{fp28_mulx(XX3.c0, xP), fp28_mulx(XX3.c1, xP)}));  // 3.33 x 256 -> 1.34; 2
  l3 = fp2_28{fp28_mulx(H.c0, yP), fp28_mulx(H.c1, yP)};                      // 22.3 x 256 -> 3.27
  const fp2_28 F = fp2_28_muls<3>(E);                                         // 112.2, limbs 3 x 2^28
  // X3' = 2 A (B - F): B - F <= 122.3, limbs 6 x 2^28, the second operand under a K at 2^31: 1.47 x 245.3 -> 1.15
  X = fp2_28_norm(fp2_28_muls<2>(fp2_28_mul<123, 31>(A, fp2_28_sub<113, 30>(B, F))));            // 2.3
  // Y3' = (B + F)^2 - 12 E^2: 243 x 243.5 -> 24.5; E^2: 74.8 x 75.4 -> 3.24, x 12 = 38.9
  Y = fp2_28_norm(fp2_28_sub<39, 30>(fp2_28_sqr<122, 28>(fp2_28_norm(fp2_28_add(B, F))),
                                     fp2_28_muls<3>(fp2_28_norm(fp2_28_muls<4>(fp2_28_sqr<38, 28>(E))))));  // 63.5
  Z = fp2_28_norm(fp2_28_muls<4>(fp2_28_mul<10, 28>(H, B)));                  // 22.3 x 19.3 -> 1.18; 4.7
}

// addition step T <- T + Q, Q's coordinates as the limbs of a 2^8 too (they meet Z, theta and lam,
// at most 75 p, at once).  Lines leave normalised: l0 <= 21, l2 <= 9, l3 <= 3.
LB_HD void miller_add28(fp2_28& X, fp2_28& Y, fp2_28& Z, const fp2_28& Qx, const fp2_28& Qy, fp2_28& l0, fp2_28& l2,
                        fp2_28& l3, const fp28& xP, const fp28& yP) {
  const fp2_28 theta = fp2_28_norm(fp2_28_sub<3, 28>(Y, fp2_28_mul<9, 28>(Qy, Z)));  // 256 x 17 -> 2.73; 75
  const fp2_28 lam = fp2_28_norm(fp2_28_sub<3, 28>(X, fp2_28_mul<9, 28>(Qx, Z)));    // 11
  // theta xQ: 256 x 151 -> 16.4; lam yQ: 256 x 23 -> 3.34; l0 <= 20.4
  l0 = fp2_28_norm(fp2_28_sub<4, 28>(fp2_28_mul<76, 28>(Qx, theta), fp2_28_mul<12, 28>(Qy, lam)));
  l2 = fp2_28_norm(fp2_28_kminus<9, 28>(fp2_28{fp28_mulx(theta.c0, xP), fp28_mulx(theta.c1, xP)}));  // 75 x 256 -> 8.62; 9
  l3 = fp2_28{fp28_mulx(lam.c0, yP), fp28_mulx(lam.c1, yP)};                   // 11 x 256 -> 2.12
  const fp2_28 C = fp2_28_sqr<76, 28>(theta);                                  // 150 x 151 -> 9.99
  const fp2_28 D = fp2_28_sqr<12, 28>(lam);                                    // 22 x 23 -> 1.21
  const fp2_28 E = fp2_28_mul<2, 28>(lam, D);                                  // 11 x 3.21 -> 1.02
  const fp2_28 F = fp2_28_mul<10, 28>(Z, C);                                   // 8 x 20 -> 1.07
  const fp2_28 G = fp2_28_mul<2, 28>(X, D);                                    // 8 x 3.21 -> 1.02
  const fp2_28 H = fp2_28_norm(fp2_28_sub<3, 29>(fp2_28_add(E, F), fp2_28_muls<2>(G)));  // 2.09 + 3 = 5.09
  X = fp2_28_mul<6, 28>(lam, H);                                               // 11 x 11.1 -> 1.05
  // theta (G - H): G - H <= 7.02, limbs 3 x 2^28, first operand: 7.02 x 151 -> 1.43; E Y: 72 x 3.02 -> 1.09
  Y = fp2_28_norm(fp2_28_sub<2, 28>(fp2_28_mul<76, 28>(fp2_28_sub<6, 28>(G, H), theta), fp2_28_mul<2, 28>(Y, E)));  // 3.43
  Z = fp2_28_mul<2, 28>(Z, E);                                                 // 1.01
}

// f <- f^2 = (c0' - t - v t) + 2 t w, t = a0 a1, c0' = (a0 + a1)(a0 + v a1).  t goes to slot 2; then
// the two operand sums overwrite f in slots 0 and 1 (normalised: their sums of two are the Karatsuba
// operands), c0' stays in registers and the results are written coefficient by coefficient.
template <class S_t>
LB_HD void f_sqr28(const S_t& S) {
  auto at = [&](int k) { return [&S, k](int i) { return S.get2(k, i); }; };
  // t = a0 a1: a <= (10, 14, 6), b <= (20, 27, 17), two of b <= 47: t0..t2 <= 1.31, the sums' products <= 1.9,
  // x <= 4.9; t <= (11.2, 8.2, 6.2)
  fp6_28_mul_to<28, 48, 3, 5, 2>(at(0), at(1), [&](int i, const fp2_28& v) { S.put2(2, i, v); });
  {
    const fp2_28 b0 = S.get2(1, 0), b1 = S.get2(1, 1), b2 = S.get2(1, 2);
    fp2_28 a = S.get2(0, 0);
    S.put2(0, 0, fp2_28_norm(fp2_28_add(a, b0)));                             // s1 = a0 + a1 <= (30, 41, 23)
    S.put2(1, 0, fp2_28_norm(fp2_28_add(a, fp2_28_mul_xi<18, 28>(b2))));      // s2 = a0 + v a1 <= (45, 34, 33)
    a = S.get2(0, 1);
    S.put2(0, 1, fp2_28_norm(fp2_28_add(a, b1)));
    S.put2(1, 1, fp2_28_norm(fp2_28_add(a, b0)));
    a = S.get2(0, 2);
    S.put2(0, 2, fp2_28_norm(fp2_28_add(a, b2)));
    S.put2(1, 2, fp2_28_norm(fp2_28_add(a, b1)));
  }
  // c0' = s1 s2: two of s2 <= 79: t0..t2 <= 2.3, the sums' products <= 5.5, x <= 9.7; c0' <= (21.9, 13.8, 12.5)
  fp6_28 c;
  fp6_28_mul_to<46, 80, 5, 10, 3>(at(0), at(1), [&](int i, const fp2_28& v) { fp6_28_at(c, i) = v; });
  {  // t + v t <= (25.4, 19.4, 14.4), limbs 4 x 2^28 in coefficient 0 and 2^29 in the others: f.c0 <= (47.8, 37.2, 27.6),
     // f.c1 = 2 t <= (21.8, 16.0, 11.7), all inside what the line product is sized for
    const fp2_28 t0 = S.get2(2, 0), t1 = S.get2(2, 1), t2 = S.get2(2, 2);
    S.put2(0, 0, fp2_28_norm(fp2_28_sub<26, 31>(c.c0, fp2_28_add(t0, fp2_28_mul_xi<8, 28>(t2)))));
    S.put2(0, 1, fp2_28_norm(fp2_28_sub<22, 29>(c.c1, fp2_28_add(t1, t0))));
    S.put2(0, 2, fp2_28_norm(fp2_28_sub<16, 29>(c.c2, fp2_28_add(t2, t1))));
    S.put2(1, 0, fp2_28_norm(fp2_28_muls<2>(t0)));
    S.put2(1, 1, fp2_28_norm(fp2_28_muls<2>(t1)));
    S.put2(1, 2, fp2_28_norm(fp2_28_muls<2>(t2)));
  }
}
// f <- f (l0 + l2 v + l3 v w), lines normalised with l0 <= 48, l2 <= 9, l3 <= 4 (fp12_mul_line_inl):
// t1 = a1 l3 v -> slot 2; s = a0 + a1 -> slot 1 (a1 is spent); t0 = a0 (l0 + l2 v) -> slot 0 in
// place; c1' = s (l0 + (l2 + l3) v) in registers; then f.c1 = c1' - t0 - t1, f.c0 = t0 + v t1.
template <class S_t>
LB_HD void f_line28(const S_t& S, const fp2_28& l0, const fp2_28& l2, const fp2_28& l3) {
  auto at = [&](int k) { return [&S, k](int i) { return S.get2(k, i); }; };
  // f <= 48 p here (after a squaring; 27 p before an addition pass).  t1: 48 x 7.3 -> 1.14; xi of it 3.14
  fp6_28_mul_1_to<4, 2>(at(1), l3, [&](int i, const fp2_28& v) { S.put2(2, i, v); });
  LB_UNROLL for (int i = 0; i < 3; i++) S.put2(1, i, fp2_28_add(S.get2(0, i), S.get2(1, i)));
  // t0: a0 l0 -> 2.8, a1 l2 -> 1.4, (a0 + a1)(l0 + l2 <= 56.3) -> 5.4; t0 <= (6.2, 10.4, 4.2), the last with limbs 2^29
  fp6_28_mul_01_to<48, 10, 57, 5, 2>(at(0), l0, l2, fp2_28_norm(fp2_28_add(l0, l2)),
                                    [&](int i, const fp2_28& v) { S.put2(0, i, v); });
  fp6_28 c;
  {
    // s <= 96, limbs 2^29: s0 l0 -> 4.6, s1 l23 -> 2.0 (l23 <= 12.3), (s0 + s1)(l0 + l23 <= 59.6) -> 10.3; c1' <= (8.6, 17.3, 6.6)
    const fp2_28 l23 = fp2_28_norm(fp2_28_add(l2, l3));
    fp6_28_mul_01_to<48, 13, 61, 7, 2>(at(1), l0, l23, fp2_28_norm(fp2_28_add(l0, l23)),
                                       [&](int i, const fp2_28& v) { fp6_28_at(c, i) = v; });
  }
  // t0 + t1 <= (9.3, 11.5, 5.3), limbs 3 x 2^28: f.c1 <= c1' + 12; f.c0 = t0 + v t1
  LB_UNROLL for (int i = 0; i < 3; i++) {
    const fp2_28 t0 = S.get2(0, i);
    S.put2(1, i, fp2_28_norm(fp2_28_sub<12, 30>(fp6_28_at(c, i), fp2_28_add(t0, S.get2(2, i)))));
    S.put2(0, i, fp2_28_norm(fp2_28_add(t0, i == 0 ? fp2_28_mul_xi<2, 28>(S.get2(2, 2)) : S.get2(2, i - 1))));
  }
}

// The loop over the slots: f_{|x|,Q}(P) before the conjugation, f left in slots 0 and 1 in limb
// form.  ldP() and ldQ() re-read the 12-word affine points wherever they are used, as the kernel
// does; one line product serves the doubling and the addition pass of a step.
template <class S_t, class LdP, class LdQ>
LB_HD void miller_lane28(const S_t& S, LdP&& ldP, LdQ&& ldQ) {
  {
    const g2a Q = ldQ();
    S.put2(3, 0, fp2_28_from_fp2(Q.x));
    S.put2(3, 1, fp2_28_from_fp2(Q.y));
    S.put2(3, 2, fp2_28{fp28_one(), fp28_zero()});
  }
  bool first = true;
#pragma clang loop unroll(disable)
  for (int i = 62; i >= 0; i--) {
    LB_CHK(miller28_chk_assume(S);)
    if (!first) f_sqr28(S);
    first = false;
    const int np = 1 + (int)((LB_X_ABS >> i) & 1ull);
#pragma clang loop unroll(disable)
    for (int pass = 0; pass < np; pass++) {
      LB_CHK(if (pass) miller28_chk_assume(S);)
      fp2_28 l0, l2, l3;
      {
        fp2_28 X = S.get2(3, 0), Y = S.get2(3, 1), Z = S.get2(3, 2);
        const g1a P = ldP();
        const fp28 xP = fp28_from_fp_shift(P.x), yP = fp28_from_fp_shift(P.y);
        if (pass == 0) {
          miller_dbl28(X, Y, Z, l0, l2, l3, xP, yP);
        } else {
          const g2a Q = ldQ();
          miller_add28(X, Y, Z, fp2_28_from_fp2_shift(Q.x), fp2_28_from_fp2_shift(Q.y), l0, l2, l3, xP, yP);
        }
        S.put2(3, 0, X), S.put2(3, 1, Y), S.put2(3, 2, Z);
      }
      f_line28(S, l0, l2, l3);
    }
  }
}

// a^|x| for a in the cyclotomic subgroup
LB_NI fp12 fp12_pow_xabs(fp12 a) {
  fp12 r = a;
  for (int i = 62; i >= 0; i--) {
    r = fp12_sqr(r);
    if ((LB_X_ABS >> i) & 1ull) r = fp12_mul(r, a);
  }
  return r;
}

// f^(3 (p^12 - 1)/r)
LB_NI fp12 final_exponentiation(fp12 f) {
  // easy part: f^((p^6 - 1)(p^2 + 1))
  fp12 t = fp12_mul(fp12_conj(f), fp12_inv(f));
  t = fp12_mul(fp12_frob2(t), t);
  // hard part: t^((x-1)^2 (x+p) (x^2+p^2-1) + 3)
  fp12 a = fp12_conj(fp12_mul(fp12_pow_xabs(t), t));  // t^(x-1)
  a = fp12_conj(fp12_mul(fp12_pow_xabs(a), a));        // t^((x-1)^2)
  fp12 b = fp12_mul(fp12_conj(fp12_pow_xabs(a)), fp12_frob(a));  // a^(x+p)
  fp12 c = fp12_pow_xabs(fp12_pow_xabs(b));                        // b^(x^2)
  c = fp12_mul(fp12_mul(c, fp12_frob2(b)), fp12_conj(b));          // b^(x^2+p^2-1)
  fp12 t3 = fp12_mul(fp12_sqr(t), t);
  return fp12_mul(c, t3);
}
