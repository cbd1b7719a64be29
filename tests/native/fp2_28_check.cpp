// Host check of the limb-resident Fp2 layer (lb_field.h fp2_28) and of the psi-ladder built on it
// (lb_curve.h g2_dbl_lean28, g2_madd_lean28, g2_aff_in_subgroup28) against the 12 x 32-bit forms.
// Built with -DLB_FP28_CHECK: every product asserts its 64-bit columns against 128-bit sums and the
// layer's worst-case bound propagation aborts where a column, borrow or value bound fails, so a
// clean run is the proof that the bounds written in lb_curve.h close.  tests/test_fp2_28_host.py
// builds it with g++, plain and with -fsanitize=address,undefined, and runs it on
// tests/golden/subgroup28_points.txt (argv[1]).  No GPU.
#ifndef LB_FP28_CHECK
#error "build with -DLB_FP28_CHECK"
#endif
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "lb_curve.h"

static int g_bad = 0, g_checks = 0;
#define EXPECT(c)                                           \
  do {                                                      \
    g_checks++;                                             \
    if (!(c)) {                                             \
      g_bad++;                                              \
      if (g_bad < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                       \
  } while (0)

static std::mt19937_64 rng(28);

static fp small_mont(uint32_t v) {
  fp a = fp_zero();
  a.v[0] = v;
  return fp_to_mont(a);
}
// the element an fp28 stands for, by a path of its own: N = sum l_k 2^(28 k) evaluated in Fp by
// Horner's rule, then N / 2^8 (N = x R', the 12-word form is x R = N / 2^8) as a plain integer
static fp ref28(const fp28& a) {
  static const fp c28 = small_mont(1u << 28);
  static const fp inv256 = fp_inv(small_mont(256));
  fp v = fp_zero();
  for (int k = 13; k >= 0; k--) v = fp_add(fp_mul(v, c28), small_mont(a.l[k]));
  return fp_from_mont(fp_mul(v, inv256));
}
static fp2 ref2(const fp2_28& a) { return fp2{ref28(a.c0), ref28(a.c1)}; }

static fp rand_fp() {
  fp a;
  for (int k = 0; k < 12; k++) a.v[k] = (uint32_t)rng();
  a.v[11] &= 0x0fffffffu;  // < 2^380 < p
  return a;
}
static fp p_minus_1() {
  fp a = fp_load(LB_P);
  a.v[0] -= 1;
  return a;
}
// an operand built directly in limb form: limbs 0..12 random up to L (or all equal to L), the top
// limb the largest that keeps the value below vb p, with exactly these bounds declared
static fp28 limb_form(uint64_t L, double vb, bool at_max) {
  fp28 a;
  for (int k = 0; k < 13; k++) a.l[k] = at_max ? (uint32_t)L : (uint32_t)(rng() % (L + 1));
  const uint64_t top = (uint64_t)(vb * 106513.0) - (L >> 28) - 2;  // value < (top + L / 2^28 + 1) 2^364 <= vb p
  a.l[13] = at_max ? (uint32_t)top : (uint32_t)(rng() % (top + 1));
  for (int k = 0; k < 13; k++) a.ub[k] = L;
  a.ub[13] = fp28_chk_top(vb);
  a.vb = vb;
  return a;
}
static fp2_28 limb_form2(uint64_t L, double vb, bool at_max) { return fp2_28{limb_form(L, vb, at_max), limb_form(L, vb, at_max)}; }
static bool normalised(const fp28& a) {
  for (int k = 0; k < 13; k++)
    if (a.l[k] >> 28) return false;
  return true;
}

#define N28 0x0fffffffull
static void field_checks() {
  // conversions and the canonical cases: 0, 1, p - 1, equal components, a1 = 0, random
  std::vector<fp> es = {fp_zero(), fp_one(), p_minus_1(), small_mont(2)};
  for (int i = 0; i < 12; i++) es.push_back(rand_fp());
  std::vector<fp2> vs;
  for (size_t i = 0; i < es.size(); i++) {
    vs.push_back(fp2{es[i], es[(i * 7 + 3) % es.size()]});
    vs.push_back(fp2{es[i], es[i]});       // both components equal
    vs.push_back(fp2{es[i], fp_zero()});   // a1 = 0
  }
  for (const fp& e : es) {
    EXPECT(fp_eq(ref28(fp28_from_fp(e)), e));
    EXPECT(fp_eq(ref28(fp28_from_fp_shift(e)), e));
    EXPECT(fp_eq(fp28_to_fp(fp28_from_fp(e)), e));
    EXPECT(fp_eq(fp28_to_fp(fp28_from_fp_shift(e)), e));
    EXPECT(fp28_is_zero(fp28_from_fp(e)) == fp_is_zero(e));
    EXPECT(fp28_is_zero(fp28_from_fp_shift(e)) == fp_is_zero(e));
  }
  EXPECT(fp_eq(fp28_to_fp(fp28_one()), fp_one()));
  EXPECT(fp28_is_zero(fp28_zero()));
  for (size_t i = 0; i < vs.size(); i++) {
    const fp2 &a = vs[i], &b = vs[(i * 5 + 1) % vs.size()];
    const fp2_28 A = fp2_28_from_fp2(a), B = fp2_28_from_fp2(b), As = fp2_28_from_fp2_shift(a);
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_mul<2, 28>(A, B)), fp2_mul(a, b)));
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_mul<2, 28>(As, B)), fp2_mul(a, b)));  // a 256 p operand against 1 p
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_sqr<2, 28>(A)), fp2_sqr(a)));
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_sub<2, 28>(A, B)), fp2_sub(a, b)));
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_add(A, B)), fp2_add(a, b)));
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_muls<8>(A)), fp2_mul8(a)));
    EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_muls<3>(A)), fp2_mul3(a)));
    const fp2_28 n = fp2_28_norm(fp2_28_muls<4>(fp2_28_sub<2, 28>(A, B)));
    EXPECT(normalised(n.c0) && normalised(n.c1));
    EXPECT(fp2_eq(fp2_28_to_fp2(n), fp2_mul4(fp2_sub(a, b))));
    EXPECT(fp2_28_is_zero(fp2_28_sub<2, 28>(A, A)));
    EXPECT(fp2_28_is_zero(fp2_28_sub<2, 28>(A, B)) == fp2_eq(a, b));
  }
  // operands at the stated limb and value bounds, in limb form: the shapes the ladder uses at their
  // maxima (all limbs at the bound) and at random below them
  for (int it = 0; it < 40; it++) {
    const bool mx = it < 2;
    {  // a wide first operand (4 x 2^28, 10.8 p: I) against a normalised 32.4 p second one (H)
      const fp2_28 a = limb_form2(4 * N28, 10.8, mx), b = limb_form2(N28, 32.4, mx);
      EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_mul<33, 28>(a, b)), fp2_mul(ref2(a), ref2(b))));
    }
    {  // 3 x 2^28 at 44.2 p (D - X3) against a normalised 7.4 p (E)
      const fp2_28 a = limb_form2(3 * N28 + 3, 44.2, mx), b = limb_form2(N28, 7.4, mx);
      EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_mul<8, 28>(a, b)), fp2_mul(ref2(a), ref2(b))));
    }
    {  // a second operand of 2^29 limbs covered by a K borrowed at 2^29
      const fp2_28 a = limb_form2(2 * N28, 20.0, mx), b = limb_form2(2 * N28, 20.0, mx);
      EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_mul<21, 29>(a, b)), fp2_mul(ref2(a), ref2(b))));
    }
    {  // the widest square: a normalised 32.4 p operand (H); and the ladder's X at 30 p
      const fp2_28 a = limb_form2(N28, 32.4, mx), x = limb_form2(N28, LB_L28_VX, mx);
      EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_sqr<33, 28>(a)), fp2_sqr(ref2(a))));
      EXPECT(fp2_eq(fp2_28_to_fp2(fp2_28_sqr<31, 28>(x)), fp2_sqr(ref2(x))));
    }
    {  // the column bound itself: two products with all four sides near 2^29.5, and 2^31 against 2^28
      const uint64_t L = 759250124;  // floor(2^29.5)
      const fp28 a = limb_form(L, 4.0, mx), b = limb_form(L, 4.0, mx), c = limb_form(L, 4.0, mx), d = limb_form(L, 4.0, mx);
      EXPECT(fp_eq(fp28_to_fp(fp28_mac2(a, b, c, d)), fp_add(fp_mul(ref28(a), ref28(b)), fp_mul(ref28(c), ref28(d)))));
      const fp28 w = limb_form((1ull << 31) - 8, 9.0, mx), n = limb_form(N28, 30.0, mx);
      EXPECT(fp_eq(fp28_to_fp(fp28_mac2(w, n, w, n)), fp_dbl(fp_mul(ref28(w), ref28(n)))));
    }
    {  // subtractions at their borrow bounds: 8 C (limbs 2^31 - 8) from a product, two stacked, 2 D
      const fp2_28 a = limb_form2(N28, 1.3, mx), c = limb_form2(N28, 1.004, mx), d = limb_form2(N28, 13.2, mx);
      const fp2_28 r = fp2_28_sub<9, 31>(a, fp2_28_muls<8>(c));
      EXPECT(fp2_eq(ref2(r), fp2_sub(ref2(a), fp2_mul8(ref2(c)))));
      const fp2_28 n = fp2_28_norm(r);
      EXPECT(normalised(n.c0) && normalised(n.c1) && fp2_eq(ref2(n), ref2(r)));
      const fp2_28 s = fp2_28_norm(fp2_28_muls<2>(fp2_28_sub<2, 28>(fp2_28_sub<2, 28>(a, c), c)));
      EXPECT(fp2_eq(ref2(s), fp2_dbl(fp2_sub(fp2_sub(ref2(a), ref2(c)), ref2(c)))));
      const fp2_28 t = fp2_28_norm(fp2_28_sub<27, 29>(a, fp2_28_muls<2>(d)));
      EXPECT(fp2_eq(ref2(t), fp2_sub(ref2(a), fp2_dbl(ref2(d)))));
      EXPECT(fp2_eq(fp2_28_to_fp2(t), ref2(t)));
    }
  }
}

struct pt {
  std::string kind;
  int expect;
  g2a a;
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
static std::vector<pt> load_points(const char* path) {
  std::vector<pt> out;
  FILE* f = fopen(path, "r");
  if (!f) return out;
  char kind[32], h[4][128];
  int e;
  while (fscanf(f, "%31s %d %127s %127s %127s %127s", kind, &e, h[0], h[1], h[2], h[3]) == 6) {
    pt p;
    p.kind = kind, p.expect = e;
    p.a.x = fp2{parse_fp(h[0]), parse_fp(h[1])};
    p.a.y = fp2{parse_fp(h[2]), parse_fp(h[3])};
    out.push_back(p);
  }
  fclose(f);
  return out;
}
static g2j28 g2j28_from_jac(const g2j& o) {
  return g2j28{fp2_28_from_fp2(o.x), fp2_28_from_fp2(o.y), fp2_28_from_fp2(o.z)};
}
static bool same_point(const g2j28& n, const g2j& o) {
  g2a a, b;
  const bool fa = jac_to_aff(a, g2j28_to_g2j(n)), fb = jac_to_aff(b, o);
  if (fa != fb) return false;
  return !fa || (fp2_eq(a.x, b.x) && fp2_eq(a.y, b.y));
}
static void ladder_checks(const std::vector<pt>& pts) {
  for (const pt& p : pts) {
    EXPECT(g2_aff_on_curve(p.a));
    auto ld = [&](int o) { return o == 0 ? p.a.x : p.a.y; };
    g2_park28 pk;
    // steps: doublings and mixed additions side by side, compared as affine points
    g2j o = jac_from_aff(p.a);
    g2j28 n = g2j28_from_aff(p.a.x, p.a.y);
    for (int s = 0; s < 10; s++) {
      g2_dbl_lean<false>(o);
      g2_dbl_lean28(n);
      EXPECT(same_point(n, o));
      if (s % 3 == 0 && !jac_is_inf(o)) {
        g2j t = o;
        g2_add_aff_lean<false>(t, p.a);
        const int e = g2_madd_lean28(n, ld, pk);
        if (e == 0) o = t;
        // p == +-q spends the state: the reference's doubling or infinity tells which; go on from o
        EXPECT(e == 0 ? same_point(n, t) : e == 2 ? jac_is_inf(t) : !jac_is_inf(t));
        if (e != 0) n = g2j28_from_jac(o);
      }
    }
    // the exceptional additions at the addition itself: acc = P and acc = -P
    g2j28 q = g2j28_from_aff(p.a.x, p.a.y);
    EXPECT(g2_madd_lean28(q, ld, pk) == 1);
    q = g2j28_from_aff(p.a.x, fp2_neg(p.a.y));
    EXPECT(g2_madd_lean28(q, ld, pk) == 2);
    // the whole |x| ladder and the psi comparison: the verdict of the current host path, and the oracle's
    const bool v28 = g2_aff_in_subgroup28(ld, pk), vold = g2_aff_in_subgroup_i(p.a);
    EXPECT(v28 == vold);
    EXPECT(v28 == (p.expect != 0));
  }
  EXPECT(g2j28_is_inf(g2j28_infinity()));
}

int main(int argc, char** argv) {
  field_checks();
  const int nf = g_checks;
  std::vector<pt> pts;
  if (argc > 1) pts = load_points(argv[1]);
  ladder_checks(pts);
  printf("points: %zu  field checks: %d  ladder checks: %d  failures: %d\n", pts.size(), nf, g_checks - nf, g_bad);
  return g_bad != 0 || pts.empty();
}
