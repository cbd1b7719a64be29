// Stand-alone check of the FK20 pieces (lb_fk20.h through tests/harness/kzg_fk20_lanes.h) for a
// sanitizer build (tests/test_kzg_fk20_cpu.py builds it with -fsanitize=address,undefined and runs it):
// the 128-point stage schedule over fr against a direct sum (forward, inverse with scale,
// inverse(forward(v)) = v, 64 live inputs); the column gather and transforms of k_fr_fk_cols against
// direct sums over the columns written out by hand (dense, X^64, X^4095, X^63); the whole pass in the
// scalar model (s[t] = tau^t) against the long-division quotient of cells 0, 1, 5, 63, 64 and 127,
// with h[63] = 0 and h[64 .. 127] not all zero; the schedule over G1 points with entries at infinity
// (outputs 0 and 64 against plain scalar multiples).  The columns of the monomials
// are checked at both ends of the residue range only; the Python harness test covers them all.  CPU only.
#include <stdio.h>
#include <vector>
#include "kzg_fk20_lanes.h"

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      failures++;                                                    \
      printf("kzg_fk20_check: FAILED line %d: %s\n", __LINE__, #c);  \
    }                                                                \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static fr rnd_fr() {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = rng32();
  return fr_reduce256(w);
}
static fr pow_u32(const fr& a, uint32_t e) {
  fr acc = fr_one(), sq = a;
  for (; e; e >>= 1, sq = fr_sqr(sq))
    if (e & 1u) acc = fr_mul(acc, sq);
  return acc;
}
static fr w128() { return pow_u32(fr_root8192(), 64); }
// out[m] = sum_j v[j] w^(j m), the plain double loop
static void direct_dft(const fr* v, const fr& w, fr* out) {
  for (uint32_t m = 0; m < 128; m++) {
    const fr wm = pow_u32(w, m);
    fr acc = fr_zero(), x = fr_one();
    for (uint32_t j = 0; j < 128; j++, x = fr_mul(x, wm)) acc = fr_add(acc, fr_mul(v[j], x));
    out[m] = acc;
  }
}
static bool same(const fr* a, const fr* b, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (!fr_eq(a[i], b[i])) return false;
  return true;
}

static void check_fr_schedule(const fr* tab) {
  fr v[128], want[128], got[128], back[128];
  for (auto& x : v) x = rnd_fr();
  direct_dft(v, w128(), want);
  fk_fft_fr_lanes(v, 128, tab, false, false, got);
  CHECK(same(got, want, 128));
  fk_fft_fr_lanes(got, 128, tab, true, true, back);
  CHECK(same(back, v, 128));
  direct_dft(v, fr_inv(w128()), want);
  fk_fft_fr_lanes(v, 128, tab, true, false, got);
  CHECK(same(got, want, 128));
  fr half[128];
  for (uint32_t j = 0; j < 128; j++) half[j] = j < 64 ? v[j] : fr_zero();
  direct_dft(half, w128(), want);
  fk_fft_fr_lanes(v, 64, tab, false, false, got);
  CHECK(same(got, want, 128));
}

static void check_cols(const std::vector<fr>& a, const fr* tab, bool expect_zero, uint32_t i_step) {
  std::vector<uint32_t> le((size_t)8 * LB_FK_POINTS, 0xAAAAAAAAu);
  fk_cols_lanes(a.data(), tab, le.data());
  const fr inv = fr_inv(fr_from_u32(128));
  bool ok = true, zero = true;
  for (uint32_t i = 0; i < 64; i += i_step) {
    fr c[128], want[128];
    c[0] = a[4095 - i];
    for (uint32_t k = 1; k < 66; k++) c[k] = fr_zero();
    for (uint32_t k = 66; k < 128; k++) c[k] = a[64 * (k - 64) - i - 1];
    direct_dft(c, w128(), want);
    for (uint32_t r = 0; r < 128; r++) {
      const fr got = fr_to_mont(fr_from_words(&le[(size_t)8 * (64 * r + i)]));
      ok &= fr_eq(got, fr_mul(want[r], inv));
      zero &= fr_is_zero(got);
    }
  }
  CHECK(ok);
  CHECK(zero == expect_zero);
}

// the whole pass with field elements for points
static void check_scalar_model(const std::vector<fr>& a, const fr* tab, bool dense) {
  const fr tau = rnd_fr();
  std::vector<fr> s(4096);
  s[0] = fr_one();
  for (uint32_t t = 1; t < 4096; t++) s[t] = fr_mul(s[t - 1], tau);
  std::vector<uint32_t> le((size_t)8 * LB_FK_POINTS);
  fk_cols_lanes(a.data(), tab, le.data());
  fr E[128];
  for (auto& x : E) x = fr_zero();
  for (uint32_t i = 0; i < 64; i++) {
    fr x[128], X[128];
    for (uint32_t j = 0; j < 128; j++) {
      const uint32_t idx = fk_setup_index(i, j);
      x[j] = idx == LB_FK_NONE ? fr_zero() : s[idx];
    }
    fk_fft_fr_lanes(x, 128, tab, false, false, X);
    for (uint32_t r = 0; r < 128; r++)
      E[r] = fr_add(E[r], fr_mul(fr_to_mont(fr_from_words(&le[(size_t)8 * (64 * r + i)])), X[r]));
  }
  fr h[128], D[128];
  fk_fft_fr_lanes(E, 128, tab, true, false, h);  // the scale is in the scalars already
  CHECK(fr_is_zero(h[63]));
  if (dense) {
    bool upper_zero = true;
    for (uint32_t j = 64; j < 128; j++) upper_zero &= fr_is_zero(h[j]);
    CHECK(!upper_zero);
  }
  fk_fft_fr_lanes(h, LB_FK_LIVE, tab, false, false, D);
  const uint32_t cells[6] = {0, 1, 5, 63, 64, 127};
  for (uint32_t ci : cells) {
    // long division by X^64 - y, y = w128^brp7(ci); the quotient's commitment sum q_u tau^u
    const fr y = pow_u32(w128(), fr_bitrev(ci, 7));
    std::vector<fr> rem(a);
    fr commit = fr_zero();
    for (uint32_t j = 4095; j >= 64; j--) {
      commit = fr_add(commit, fr_mul(rem[j], s[j - 64]));
      rem[j - 64] = fr_add(rem[j - 64], fr_mul(y, rem[j]));
    }
    CHECK(fr_eq(D[fr_bitrev(ci, 7)], commit));
  }
}

static void check_g1(const fr* tab) {
  const g1a g{fp_load(LB_G1X), fp_load(LB_G1Y)};
  std::vector<g1j> in(128), out(128);
  uint64_t k[128], sum = 0;
  fr alt = fr_zero();
  for (uint32_t j = 0; j < 128; j++) {
    k[j] = (j == 0 || j == 7 || j == 64 || j == 127) ? 0 : 1 + (rng32() & 0xfffffu);
    in[j] = k[j] ? jac_mul_u64(g, k[j]) : jac_infinity<fp>();
    sum += k[j];
    const fr kj = fr_from_u32((uint32_t)k[j]);
    alt = (j & 1u) ? fr_sub(alt, kj) : fr_add(alt, kj);  // w128^64 = -1
  }
  fk_fft_g1_lanes(in.data(), 128, tab, false, false, out.data());
  CHECK(jac_eq(out[0], jac_mul_u64(g, sum)));
  uint32_t aw[8];
  fr_to_le_words(aw, alt);
  CHECK(jac_eq(out[64], jac_mul_u255_jac(jac_from_aff(g), aw)));
}

int main() {
  std::vector<fr> tab(LB_FK_TAB_LEN);
  fk_tables(tab.data());
  CHECK(fr_eq(tab[LB_FK_TAB_FWD_MONT + 1], w128()));
  CHECK(fr_eq(fr_mul(tab[LB_FK_TAB_FWD_MONT + 5], tab[LB_FK_TAB_INV_MONT + 5]), fr_one()));
  check_fr_schedule(tab.data());
  std::vector<fr> dense(4096), mono(4096, fr_zero());
  for (auto& x : dense) x = rnd_fr();
  check_cols(dense, tab.data(), false, 1);
  const uint32_t degs[3] = {64, 4095, 63};
  for (uint32_t d : degs) {
    mono.assign(4096, fr_zero());
    mono[d] = fr_one();
    check_cols(mono, tab.data(), d == 63, 63);
    check_scalar_model(mono, tab.data(), false);
  }
  check_scalar_model(dense, tab.data(), true);
  std::vector<fr> d70(4096, fr_zero());
  for (uint32_t j = 0; j <= 70; j++) d70[j] = rnd_fr();
  check_scalar_model(d70, tab.data(), false);
  check_g1(tab.data());
  printf("kzg_fk20_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
