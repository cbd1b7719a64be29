// Stand-alone check of the batched KZG verification's per-lane pieces (lb_fr.h fr_seg_aggregate,
// fr_eq_local + fr_ev_weight + fr_ev_fold) for a sanitizer build (tests/test_kzg_batch_cpu.py builds
// it with -fsanitize=address,undefined and runs it): the segmented aggregation for the offsets
// 0,0,1,3,3,4 against a plain double loop, and the evaluation of 4096-coefficient polynomials
// against Horner at a random point, 0, 1 and a 4096th root of unity, for a random polynomial, the
// zero polynomial and one whose only coefficient is the last.  CPU only.
#include <stdio.h>
#include <vector>
#include "lb_fr.h"

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      failures++;                                                      \
      printf("kzg_batch_check: FAILED line %d: %s\n", __LINE__, #c);   \
    }                                                                  \
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
struct polys {
  const fr* p;
  uint32_t len;
  const fr& operator()(uint32_t j, uint32_t i) const { return p[(size_t)j * len + i]; }
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

// the phases of k_fr_eval_many, the lanes in turn
static fr eval_lanes(std::vector<fr>& a, const fr& z) {
  const uint32_t lanes = (uint32_t)a.size() / 4;
  std::vector<fr> v(lanes);
  flat A{a.data()}, V{v.data()};
  for (uint32_t t = 0; t < lanes; t++) V.st(t, fr_eq_local(A, z, t));
  int steps = 0;
  while ((1u << steps) < lanes) steps++;
  for (int s = steps - 1; s >= 0; s--) {
    const fr w = fr_ev_weight(z, s);
    for (uint32_t t = 0; t < lanes; t++) fr_ev_fold(V, 1u << s, w, t);
  }
  return V.ld(0);
}

int main() {
  const uint32_t n = 4096;
  // segmented aggregation: sidecars of 0, 1, 2, 0 and 1 polynomials
  {
    const uint32_t off[6] = {0, 0, 1, 3, 3, 4}, ns = 5, np = 4, len = 64;
    std::vector<fr> p((size_t)np * len), pw(np);
    for (fr& v : p) v = rnd_fr();
    for (fr& v : pw) v = rnd_fr();
    for (uint32_t k = 0; k < ns; k++)
      for (uint32_t i = 0; i < len; i++) {
        fr exp = fr_zero();
        for (uint32_t j = off[k]; j < off[k + 1]; j++) exp = fr_add(exp, fr_mul(pw[j], p[(size_t)j * len + i]));
        const fr got = fr_seg_aggregate(polys{p.data(), len}, table{pw.data()}, off[k], off[k + 1], i);
        CHECK(fr_eq(got, exp));
        if (off[k] == off[k + 1]) CHECK(fr_is_zero(got));
      }
  }
  // evaluation
  const uint32_t rw[8] = LB_FR_ROOT4096_WORDS;
  const fr root = fr_to_mont(fr_from_words(rw));
  fr root5 = fr_one();
  for (int i = 0; i < 5; i++) root5 = fr_mul(root5, root);
  std::vector<fr> rnd(n), zero(n, fr_zero()), last(n, fr_zero());
  for (fr& v : rnd) v = rnd_fr();
  last[n - 1] = rnd_fr();
  const fr zs[] = {rnd_fr(), fr_zero(), fr_one(), root5};
  for (const fr& z : zs) {
    CHECK(fr_eq(eval_lanes(rnd, z), horner(rnd, z)));
    CHECK(fr_is_zero(eval_lanes(zero, z)));
    CHECK(fr_eq(eval_lanes(last, z), horner(last, z)));
  }
  CHECK(fr_eq(eval_lanes(rnd, fr_zero()), rnd[0]));
  CHECK(fr_eq(eval_lanes(last, root5), fr_mul(last[n - 1], fr_inv(root5))));  // w^4095 = 1 / w
  // the step weights: z^(4 * 2^s)
  {
    const fr z = zs[0];
    fr w = fr_sqr(fr_sqr(z));
    for (int s = 0; s < 10; s++) {
      CHECK(fr_eq(fr_ev_weight(z, s), w));
      w = fr_sqr(w);
    }
  }
  printf("kzg_batch_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
