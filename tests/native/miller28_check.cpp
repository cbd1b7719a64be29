// Host check of the limb-resident per-root Miller loop (lb_field.h fp6_28, lb_pairing.h miller_dbl28,
// miller_add28, f_sqr28, f_line28, miller_lane28) against the 12 x 32-bit forms.  Built with
// -DLB_FP28_CHECK: every product asserts its 64-bit columns against 128-bit sums, and the layer
// propagates worst-case limb and value bounds from the loop invariant re-assumed at the top of every
// step and before every addition pass, aborting where a column, borrow or value bound fails; so a
// clean run is the proof that the bounds written in lb_pairing.h close.
// tests/test_miller28_host.py builds it with g++, plain and with -fsanitize=address,undefined, and
// runs it on tests/golden/miller28_pairs.txt (argv[1]).  "bounds" as argv[2] also prints the
// worst-case value bounds a step leaves, per coefficient.  No GPU.
#ifndef LB_FP28_CHECK
#error "build with -DLB_FP28_CHECK"
#endif
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "lb_pairing.h"

static int g_bad = 0, g_checks = 0;
#define EXPECT(c)                                           \
  do {                                                      \
    g_checks++;                                             \
    if (!(c)) {                                             \
      g_bad++;                                              \
      if (g_bad < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                       \
  } while (0)

static std::mt19937_64 rng(2812);

// the kernel's four slots of three fp2_28, with the check build's bounds beside the limbs
struct host_slots {
  mutable fp2_28 s[4][3];
  fp2_28 get2(int k, int i) const { return s[k][i]; }
  void put2(int k, int i, const fp2_28& v) const { s[k][i] = v; }
};
static void f_init(const host_slots& S) {
  for (int k = 0; k < 2; k++)
    for (int i = 0; i < 3; i++) S.put2(k, i, fp2_28{k == 0 && i == 0 ? fp28_one() : fp28_zero(), fp28_zero()});
}
static fp6 down6(const host_slots& S, int k) {
  return fp6{fp2_28_to_fp2(S.get2(k, 0)), fp2_28_to_fp2(S.get2(k, 1)), fp2_28_to_fp2(S.get2(k, 2))};
}
static fp12 down12(const host_slots& S) { return fp12{down6(S, 0), down6(S, 1)}; }
static bool fp6_eq(const fp6& a, const fp6& b) { return fp2_eq(a.c0, b.c0) && fp2_eq(a.c1, b.c1) && fp2_eq(a.c2, b.c2); }
static bool words_eq(const fp12& a, const fp12& b) { return memcmp(&a, &b, sizeof(fp12)) == 0; }

// an operand in limb form at declared bounds: limbs 0..12 up to L, the value below vb p
static fp28 limb_form(uint64_t L, double vb, bool at_max) {
  fp28 a;
  for (int k = 0; k < 13; k++) a.l[k] = at_max ? (uint32_t)L : (uint32_t)(rng() % (L + 1));
  const uint64_t top = (uint64_t)(vb * 106513.0) - (L >> 28) - 2;
  a.l[13] = at_max ? (uint32_t)top : (uint32_t)(rng() % (top + 1));
  for (int k = 0; k < 13; k++) a.ub[k] = L;
  a.ub[13] = fp28_chk_top(vb);
  a.vb = vb;
  return a;
}
static fp2_28 limb_form2(double vb, bool mx) { return fp2_28{limb_form(0x0fffffffull, vb, mx), limb_form(0x0fffffffull, vb, mx)}; }
static fp6_28 limb_form6(double v0, double v1, double v2, bool mx) {
  return fp6_28{limb_form2(v0, mx), limb_form2(v1, mx), limb_form2(v2, mx)};
}
static fp6 down(const fp6_28& a) { return fp6{fp2_28_to_fp2(a.c0), fp2_28_to_fp2(a.c1), fp2_28_to_fp2(a.c2)}; }

// the Fp6 layer on values, at the bounds of its call sites (all limbs at the maximum, then random)
static void tower_checks() {
  for (int it = 0; it < 24; it++) {
    const bool mx = it < 2;
    {  // t = a0 a1 of the squaring
      const fp6_28 a = limb_form6(LB_M28_VF00, LB_M28_VF01, LB_M28_VF02, mx), b = limb_form6(LB_M28_VF10, LB_M28_VF11, LB_M28_VF12, mx);
      EXPECT(fp6_eq(down(fp6_28_mul<28, 48, 3, 5, 2>(a, b)), fp6_mul_inl(down(a), down(b))));
      EXPECT(fp6_eq(down(fp6_28_add(a, b)), fp6_add(down(a), down(b))));
      EXPECT(fp6_eq(down(fp6_28_sub<28, 28>(a, b)), fp6_sub(down(a), down(b))));
      EXPECT(fp6_eq(down(fp6_28_mul_v<18, 28>(b)), fp6_mul_v(down(b))));
      const fp6_28 n = fp6_28_norm(fp6_28_sub<28, 28>(a, b));
      EXPECT(fp6_eq(down(n), fp6_sub(down(a), down(b))));
    }
    {  // the sparse products of the line at the doubling's line bounds
      const fp6_28 a = limb_form6(40.0, 40.0, 40.0, mx);
      const fp2_28 l0 = limb_form2(47.5, mx), l2 = limb_form2(9.0, mx), l3 = limb_form2(3.5, mx);
      EXPECT(fp6_eq(down(fp6_28_mul_01<48, 10, 57, 5, 2>(a, l0, l2)), fp6_mul_01(down(a), fp2_28_to_fp2(l0), fp2_28_to_fp2(l2))));
      EXPECT(fp6_eq(down(fp6_28_mul_1<4, 2>(a, l3)), fp6_mul_1(down(a), fp2_28_to_fp2(l3))));
    }
  }
}

struct pr {
  std::string kind;
  g1a P;
  g2a Q;
};
static fp parse_fp(const char* hex) {  // 96 hex digits, plain integer -> Montgomery words
  fp a = fp_zero();
  for (int i = 0; i < 96; i++) {
    const char c = hex[95 - i];
    const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    a.v[i / 8] |= d << (4 * (i % 8));
  }
  return fp_to_mont(a);
}
static std::vector<pr> load_pairs(const char* path) {
  std::vector<pr> out;
  FILE* f = fopen(path, "r");
  if (!f) return out;
  char kind[32], h[6][128];
  while (fscanf(f, "%31s %127s %127s %127s %127s %127s %127s", kind, h[0], h[1], h[2], h[3], h[4], h[5]) == 7) {
    pr p;
    p.kind = kind;
    p.P.x = parse_fp(h[0]), p.P.y = parse_fp(h[1]);
    p.Q.x = fp2{parse_fp(h[2]), parse_fp(h[3])};
    p.Q.y = fp2{parse_fp(h[4]), parse_fp(h[5])};
    out.push_back(p);
  }
  fclose(f);
  return out;
}

// the kernel's loop and its tail: f = 1, the limb-form loop, the conjugation, 12 conversions down
static fp12 miller28(const pr& p) {
  host_slots S;
  f_init(S);
  miller_lane28(S, [&]() { return p.P; }, [&]() { return p.Q; });
  for (int i = 0; i < 3; i++) S.put2(1, i, fp2_28_kminus<LB_M28_CONJ_C, 28>(S.get2(1, i)));
  return down12(S);
}
static void step_checks(const pr& p) {  // the first steps one by one against the 12-word forms
  host_slots S;
  f_init(S);
  S.put2(3, 0, fp2_28_from_fp2(p.Q.x)), S.put2(3, 1, fp2_28_from_fp2(p.Q.y)), S.put2(3, 2, fp2_28{fp28_one(), fp28_zero()});
  g2j T{p.Q.x, p.Q.y, fp2_one()};
  fp12 f = fp12_one();
  const fp28 xP = fp28_from_fp_shift(p.P.x), yP = fp28_from_fp_shift(p.P.y);
  for (int s = 0; s < 3; s++) {
    fp2 l0, l2, l3;
    fp2_28 m0, m2, m3;
    fp2_28 X = S.get2(3, 0), Y = S.get2(3, 1), Z = S.get2(3, 2);
    if (s) f = fp12_sqr_inl(f), f_sqr28(S);
    EXPECT(words_eq(down12(S), f));
    if (s < 2) {
      miller_dbl(T, l0, l2, l3, p.P.x, p.P.y);
      miller_dbl28(X, Y, Z, m0, m2, m3, xP, yP);
    } else {
      miller_add(T, p.Q, l0, l2, l3, p.P.x, p.P.y);
      miller_add28(X, Y, Z, fp2_28_from_fp2_shift(p.Q.x), fp2_28_from_fp2_shift(p.Q.y), m0, m2, m3, xP, yP);
    }
    EXPECT(fp2_eq(fp2_28_to_fp2(m0), l0) && fp2_eq(fp2_28_to_fp2(m2), l2) && fp2_eq(fp2_28_to_fp2(m3), l3));
    EXPECT(fp2_eq(fp2_28_to_fp2(X), T.x) && fp2_eq(fp2_28_to_fp2(Y), T.y) && fp2_eq(fp2_28_to_fp2(Z), T.z));
    S.put2(3, 0, X), S.put2(3, 1, Y), S.put2(3, 2, Z);
    f = fp12_mul_line_inl(f, l0, l2, l3);
    f_line28(S, m0, m2, m3);
    EXPECT(words_eq(down12(S), f));
  }
}

// what a step leaves, worst case: from the invariant through squaring, doubling and line, then
// through an addition pass (the figures DESIGN 5.9 quotes)
static void print_bounds(const pr& p) {
  host_slots S;
  f_init(S);
  S.put2(3, 0, fp2_28_from_fp2(p.Q.x)), S.put2(3, 1, fp2_28_from_fp2(p.Q.y)), S.put2(3, 2, fp2_28{fp28_one(), fp28_zero()});
  const fp28 xP = fp28_from_fp_shift(p.P.x), yP = fp28_from_fp_shift(p.P.y);
  auto show = [&](const char* what) {
    printf("%-22s f:", what);
    for (int k = 0; k < 2; k++)
      for (int i = 0; i < 3; i++) printf(" %6.2f", S.s[k][i].c0.vb > S.s[k][i].c1.vb ? S.s[k][i].c0.vb : S.s[k][i].c1.vb);
    printf("   T:");
    for (int i = 0; i < 3; i++) printf(" %6.2f", S.s[3][i].c0.vb > S.s[3][i].c1.vb ? S.s[3][i].c0.vb : S.s[3][i].c1.vb);
    printf("\n");
  };
  miller28_chk_assume(S);
  show("invariant");
  f_sqr28(S);
  show("after the squaring");
  fp2_28 l0, l2, l3;
  fp2_28 X = S.get2(3, 0), Y = S.get2(3, 1), Z = S.get2(3, 2);
  miller_dbl28(X, Y, Z, l0, l2, l3, xP, yP);
  S.put2(3, 0, X), S.put2(3, 1, Y), S.put2(3, 2, Z);
  printf("doubling's lines       l0 %.2f  l2 %.2f  l3 %.2f\n", l0.c0.vb, l2.c0.vb, l3.c0.vb);
  f_line28(S, l0, l2, l3);
  show("after doubling + line");
  miller28_chk_assume(S);
  X = S.get2(3, 0), Y = S.get2(3, 1), Z = S.get2(3, 2);
  miller_add28(X, Y, Z, fp2_28_from_fp2_shift(p.Q.x), fp2_28_from_fp2_shift(p.Q.y), l0, l2, l3, xP, yP);
  S.put2(3, 0, X), S.put2(3, 1, Y), S.put2(3, 2, Z);
  printf("addition's lines       l0 %.2f  l2 %.2f  l3 %.2f\n", l0.c0.vb, l2.c0.vb, l3.c0.vb);
  f_line28(S, l0, l2, l3);
  show("after addition + line");
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  tower_checks();
  const int nt = g_checks;
  std::vector<pr> prs;
  if (argc > 1) prs = load_pairs(argv[1]);
  if (argc > 2 && !strcmp(argv[2], "bounds") && !prs.empty()) print_bounds(prs[0]);
  for (const pr& p : prs) {
    step_checks(p);
    // all 144 canonical words of the leaf the kernel writes
    EXPECT(words_eq(miller28(p), miller_loop_inl(p.P, p.Q)));
  }
  printf("pairs: %zu  tower checks: %d  loop checks: %d  failures: %d\n", prs.size(), nt, g_checks - nt, g_bad);
  return g_bad != 0 || prs.empty();
}
