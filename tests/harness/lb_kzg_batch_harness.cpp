// CPU harness of the per-lane pieces of the batched KZG verification (lb_fr.h fr_seg_aggregate,
// fr_eq_local + fr_ev_weight + fr_ev_fold: what k_fr_aggregate_seg and k_fr_eval_many run), compiled
// as plain C++ for tests/test_kzg_batch_cpu.py.  Values cross the boundary as 32 little-endian
// bytes, plain form.  Test infrastructure only; the product path is the HIP build.
#include <string.h>
#include <vector>
#include "lb_fr.h"

static fr rd(const uint8_t* b) {
  fr p;
  for (int w = 0; w < 8; w++)
    p.l[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
  return fr_to_mont(p);
}
static void wr(uint8_t* b, const fr& a) {
  uint32_t w[8];
  fr_to_le_words(w, a);
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) b[4 * k + s] = (uint8_t)(w[k] >> (8 * s));
}

namespace {
struct flat {
  fr* p;
  fr ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const fr& v) { p[i] = v; }
};
struct polys {
  const fr* p;
  uint32_t len;
  const fr& operator()(uint32_t j, uint32_t i) const { return p[(size_t)j * len + i]; }
};
struct table {
  const fr* p;
  const fr& operator()(uint32_t k) const { return p[k]; }
};
}  // namespace

extern "C" {
// agg[k][i] = sum_j pw[j] poly[j][i] over sidecar k's polynomials off[k] .. off[k + 1] - 1, every
// (k, i) in turn as k_fr_aggregate_seg's threads take them.  poly: off[n] x len values, pw: off[n],
// agg: n x len.
void c_fr_aggregate_seg(uint32_t n, const uint32_t* off, uint32_t len, const uint8_t* poly32, const uint8_t* pw32,
                        uint8_t* agg32) {
  const uint32_t n_polys = off[n];
  std::vector<fr> p((size_t)n_polys * len), pw(n_polys);
  for (size_t i = 0; i < p.size(); i++) p[i] = rd(poly32 + 32 * i);
  for (uint32_t j = 0; j < n_polys; j++) pw[j] = rd(pw32 + 32 * j);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t hi = off[k + 1] < n_polys ? off[k + 1] : n_polys, lo = off[k] < hi ? off[k] : hi;
    for (uint32_t i = 0; i < len; i++)
      wr(agg32 + 32 * ((size_t)k * len + i), fr_seg_aggregate(polys{p.data(), len}, table{pw.data()}, lo, hi, i));
  }
}
// y = p(z) for n coefficients (n / 4 a power of two): the phases of k_fr_eval_many, the lanes run
// in turn within each.
void c_fr_eval(uint32_t n, const uint8_t* coeffs, const uint8_t* z32, uint8_t* y32) {
  const uint32_t lanes = n / 4;
  std::vector<fr> a(n), v(lanes);
  for (uint32_t i = 0; i < n; i++) a[i] = rd(coeffs + 32 * i);
  const fr z = rd(z32);
  flat A{a.data()}, V{v.data()};
  for (uint32_t t = 0; t < lanes; t++) V.st(t, fr_eq_local(A, z, t));
  int steps = 0;
  while ((1u << steps) < lanes) steps++;
  for (int s = steps - 1; s >= 0; s--) {
    const fr w = fr_ev_weight(z, s);
    for (uint32_t t = 0; t < lanes; t++) fr_ev_fold(V, 1u << s, w, t);
  }
  wr(y32, V.ld(0));
}
}
