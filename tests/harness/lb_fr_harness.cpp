// CPU harness of the scalar field (lb_fr.h: the field operations, the radix-2 transform and the
// evaluate-and-divide scan that the k_fr_* kernels of lb_kzg_field.h run), compiled as plain C++
// for tests/test_fr_cpu.py.  Values cross the boundary as 32 little-endian bytes, plain form.
// Test infrastructure only; the product path is the HIP build.
#include <string.h>
#include <vector>
#include "lb_fr.h"

static fr rd(const uint8_t* b) {
  fr p;
  for (int w = 0; w < 8; w++)
    p.l[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
  return fr_to_mont(p);
}
static void wr_words(uint8_t* b, const uint32_t w[8]) {
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) b[4 * k + s] = (uint8_t)(w[k] >> (8 * s));
}
static void wr(uint8_t* b, const fr& a) {
  uint32_t w[8];
  fr_to_le_words(w, a);
  wr_words(b, w);
}

namespace {
struct flat {
  fr* p;
  fr ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const fr& v) { p[i] = v; }
};
struct table {
  const fr* p;
  const fr& operator()(uint32_t k) const { return p[k]; }
};
}  // namespace

extern "C" {
// op: 0 mul, 1 add, 2 sub, 3 neg, 4 inv, 5 sqr
void c_fr_op(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
  const fr a = rd(a32), b = rd(b32);
  fr o = fr_zero();
  switch (op) {
    case 0: o = fr_mul(a, b); break;
    case 1: o = fr_add(a, b); break;
    case 2: o = fr_sub(a, b); break;
    case 3: o = fr_neg(a); break;
    case 4: o = fr_inv(a); break;
    case 5: o = fr_sqr(a); break;
  }
  wr(out32, o);
}
// a^e, e a plain 256-bit integer
void c_fr_pow(const uint8_t* a32, const uint8_t* e32, uint8_t* out32) {
  uint32_t e[8];
  for (int w = 0; w < 8; w++)
    e[w] = (uint32_t)e32[4 * w] | ((uint32_t)e32[4 * w + 1] << 8) | ((uint32_t)e32[4 * w + 2] << 16) | ((uint32_t)e32[4 * w + 3] << 24);
  wr(out32, fr_pow(rd(a32), e));
}
// 32 big-endian bytes -> the value mod r (little endian); returns 1 if it was below r
int c_fr_from_be32(const uint8_t* be32, uint8_t* out32) {
  fr a;
  const bool ok = fr_from_be32(a, be32);
  wr(out32, a);
  return ok ? 1 : 0;
}
void c_fr_reduce256(const uint8_t* in32, uint8_t* out32) {
  uint32_t w[8];
  for (int k = 0; k < 8; k++)
    w[k] = (uint32_t)in32[4 * k] | ((uint32_t)in32[4 * k + 1] << 8) | ((uint32_t)in32[4 * k + 2] << 16) | ((uint32_t)in32[4 * k + 3] << 24);
  wr(out32, fr_reduce256(w));
}
// kzg.py _ntt(a, roots) with roots[k] = root^k, in place over n = 2^logn values
void c_fr_ntt(int logn, uint8_t* data, const uint8_t* root32) {
  const uint32_t n = 1u << logn, half = n / 2;
  std::vector<fr> a(n), tw(half ? half : 1);
  for (uint32_t i = 0; i < n; i++) a[i] = rd(data + 32 * i);
  const fr w = rd(root32);
  tw[0] = fr_one();
  for (uint32_t k = 1; k < half; k++) tw[k] = fr_mul(tw[k - 1], w);
  flat A{a.data()};
  table T{tw.data()};
  fr_ntt_bitrev(A, logn, 0, 1);
  for (int s = 0; s < logn; s++) fr_ntt_stage(A, logn, s, T, 0, 1);
  for (uint32_t i = 0; i < n; i++) wr(data + 32 * i, a[i]);
}
// evaluations at the bit-reversed roots of the order-n subgroup -> monomial coefficients, the
// way k_fr_intt4096 does it: no reversal, stages over fr_intt_table, times 1 / n.  `nthr` lanes
// take turns within each phase (1 = serial; 1024 = the kernel's split of the work at logn 12).
void c_fr_intt_brp(int logn, uint8_t* data, uint32_t nthr) {
  const uint32_t n = 1u << logn, half = n / 2;
  std::vector<fr> a(n), tw(LB_FR_INTT_TABLE_LEN(logn));
  for (uint32_t i = 0; i < n; i++) a[i] = rd(data + 32 * i);
  fr_intt_table(tw.data(), logn);
  flat A{a.data()};
  table T{tw.data()};
  for (int s = 0; s < logn; s++)
    for (uint32_t t = 0; t < nthr; t++) fr_ntt_stage(A, logn, s, T, t, nthr);
  for (uint32_t i = 0; i < n; i++) wr(data + 32 * i, fr_mul(a[i], tw[half]));
}
// y = p(z) and q = (p - y) / (X - z) for n coefficients (n a multiple of 4, n / 4 a power of
// two): the phases of k_fr_eval_quotient, the lanes run in turn.  q32 holds n values (the last 0).
void c_fr_eval_quotient(uint32_t n, const uint8_t* coeffs, const uint8_t* z32, uint8_t* q32, uint8_t* y32) {
  const uint32_t lanes = n / 4;
  std::vector<fr> a(n), buf0(lanes), buf1(lanes);
  for (uint32_t i = 0; i < n; i++) a[i] = rd(coeffs + 32 * i);
  const fr z = rd(z32);
  flat A{a.data()};
  fr* src = buf0.data();
  fr* dst = buf1.data();
  for (uint32_t t = 0; t < lanes; t++) src[t] = fr_eq_local(A, z, t);
  fr w = fr_eq_weight(z);
  for (uint32_t d = 1; d < lanes; d *= 2) {
    for (uint32_t t = 0; t < lanes; t++) dst[t] = fr_eq_scan(src, lanes, d, w, t);
    fr* x = src;
    src = dst;
    dst = x;
    w = fr_sqr(w);
  }
  std::vector<uint32_t> q((size_t)8 * n);
  uint32_t y[8];
  for (uint32_t t = 0; t < lanes; t++) fr_eq_finish(A, z, src, lanes, t, q.data(), y);
  for (uint32_t i = 0; i < n; i++) wr_words(q32 + 32 * i, &q[(size_t)8 * i]);
  wr_words(y32, y);
}
}
