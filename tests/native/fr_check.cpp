// Stand-alone check of lb_fr.h for a sanitizer build (tests/test_fr_cpu.py builds it with
// -fsanitize=address,undefined and runs it): field identities on edge and pseudo-random values,
// the 4096-point transform (forward against direct evaluation, then back through the inverse form
// the kernel runs), and the evaluate-and-divide scan against Horner.  CPU only.
#include <stdio.h>
#include <vector>
#include "lb_fr.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      failures++;                                                 \
      printf("fr_check: FAILED line %d: %s\n", __LINE__, #c);     \
    }                                                             \
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

struct flat {
  fr* p;
  fr ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const fr& v) { p[i] = v; }
};
struct table {
  const fr* p;
  const fr& operator()(uint32_t k) const { return p[k]; }
};

static fr horner(const std::vector<fr>& a, const fr& z) {
  fr y = fr_zero();
  for (size_t k = a.size(); k-- > 0;) y = fr_add(fr_mul(y, z), a[k]);
  return y;
}

int main() {
  const uint32_t mod[8] = LB_FR_MOD_WORDS;
  // r - 1 and r as big-endian bytes
  uint8_t be[32];
  for (int w = 0; w < 8; w++)
    for (int s = 0; s < 4; s++) be[31 - (4 * w + s)] = (uint8_t)(mod[w] >> (8 * s));
  fr x;
  CHECK(!fr_from_be32(x, be) && fr_is_zero(x));  // r itself: rejected, reduces to 0
  be[31] = 0;                                    // r - 1
  CHECK(fr_from_be32(x, be) && fr_eq(x, fr_neg(fr_one())));
  for (int i = 0; i < 32; i++) be[i] = 0xff;
  CHECK(!fr_from_be32(x, be));
  {
    uint32_t w[8];
    for (int i = 0; i < 8; i++) w[i] = 0xffffffffu;  // 2^256 - 1 = 2^256 mod r - 1
    CHECK(fr_eq(fr_add(fr_reduce256(w), fr_one()), fr_to_mont(fr_one())));
    CHECK(fr_is_zero(fr_reduce256(mod)));
  }
  std::vector<fr> vals = {fr_zero(), fr_one(), fr_from_u32(2), fr_neg(fr_one()), fr_neg(fr_from_u32(2))};
  for (int i = 0; i < 64; i++) vals.push_back(rnd_fr());
  for (size_t i = 0; i < vals.size(); i++) {
    const fr a = vals[i], b = vals[(i * 7 + 3) % vals.size()], c = vals[(i * 5 + 1) % vals.size()];
    CHECK(fr_eq(fr_sub(fr_add(a, b), b), a));
    CHECK(fr_is_zero(fr_add(a, fr_neg(a))));
    CHECK(fr_eq(fr_mul(a, fr_add(b, c)), fr_add(fr_mul(a, b), fr_mul(a, c))));
    CHECK(fr_eq(fr_mul(a, b), fr_mul(b, a)));
    CHECK(fr_eq(fr_sqr(a), fr_mul(a, a)));
    CHECK(fr_eq(fr_to_mont(fr_from_mont(a)), a));
    CHECK(fr_lt_mod(fr_from_mont(a)));
    if (!fr_is_zero(a)) CHECK(fr_eq(fr_mul(a, fr_inv(a)), fr_one()));
    uint32_t w[8];
    fr_to_le_words(w, a);
    CHECK(fr_eq(fr_reduce256(w), a));
  }
  CHECK(fr_is_zero(fr_inv(fr_zero())));

  // the 4096-point transform
  const int logn = 12;
  const uint32_t n = 1u << logn, half = n / 2;
  std::vector<fr> inv_tw(LB_FR_INTT_TABLE_LEN(logn)), fwd_tw(half), coeffs(n), work(n);
  fr_intt_table(inv_tw.data(), logn);
  const fr w1 = fr_inv(inv_tw[1]);  // the primitive root
  fwd_tw[0] = fr_one();
  for (uint32_t k = 1; k < half; k++) fwd_tw[k] = fr_mul(fwd_tw[k - 1], w1);
  CHECK(fr_eq(fr_mul(fwd_tw[half - 1], w1), fr_neg(fr_one())));  // w^(n/2) = -1
  CHECK(fr_eq(fr_mul(inv_tw[half], fr_from_u32(n)), fr_one()));
  for (uint32_t i = 0; i < n; i++) coeffs[i] = rnd_fr();
  work = coeffs;
  flat A{work.data()};
  fr_ntt_bitrev(A, logn, 0, 1);
  for (int s = 0; s < logn; s++) fr_ntt_stage(A, logn, s, table{fwd_tw.data()}, 0, 1);
  const uint32_t at[] = {0, 1, 2, half, n - 1};
  for (uint32_t k : at) {
    const fr z = k < half ? fwd_tw[k] : fr_neg(fwd_tw[k - half]);
    CHECK(fr_eq(work[k], horner(coeffs, z)));
  }
  // values in bit-reversed order (a blob's layout) -> back to the coefficients, 1024 lanes in turn
  std::vector<fr> blob(n);
  for (uint32_t i = 0; i < n; i++) blob[i] = work[fr_bitrev(i, logn)];
  flat B{blob.data()};
  for (int s = 0; s < logn; s++)
    for (uint32_t t = 0; t < 1024; t++) fr_ntt_stage(B, logn, s, table{inv_tw.data()}, t, 1024);
  int bad = 0;
  for (uint32_t i = 0; i < n; i++) bad += !fr_eq(fr_mul(blob[i], inv_tw[half]), coeffs[i]);
  CHECK(bad == 0);

  // evaluate and divide
  const uint32_t lanes = n / 4;
  const fr zs[] = {fr_zero(), fr_one(), fwd_tw[5], rnd_fr()};
  for (const fr& z : zs) {
    std::vector<fr> b0(lanes), b1(lanes);
    fr* src = b0.data();
    fr* dst = b1.data();
    flat C{coeffs.data()};
    for (uint32_t t = 0; t < lanes; t++) src[t] = fr_eq_local(C, z, t);
    fr w = fr_eq_weight(z);
    for (uint32_t d = 1; d < lanes; d *= 2) {
      for (uint32_t t = 0; t < lanes; t++) dst[t] = fr_eq_scan(src, lanes, d, w, t);
      fr* sw = src;
      src = dst;
      dst = sw;
      w = fr_sqr(w);
    }
    std::vector<uint32_t> q((size_t)8 * n);
    uint32_t y[8];
    for (uint32_t t = 0; t < lanes; t++) fr_eq_finish(C, z, src, lanes, t, q.data(), y);
    const fr yv = fr_reduce256(y);
    CHECK(fr_eq(yv, horner(coeffs, z)));
    std::vector<fr> qv(n);
    for (uint32_t i = 0; i < n; i++) qv[i] = fr_reduce256(&q[(size_t)8 * i]);
    CHECK(fr_is_zero(qv[n - 1]));
    const fr t = rnd_fr();  // q(t) (t - z) == p(t) - y
    CHECK(fr_eq(fr_mul(horner(qv, t), fr_sub(t, z)), fr_sub(horner(coeffs, t), yv)));
  }
  printf("fr_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
