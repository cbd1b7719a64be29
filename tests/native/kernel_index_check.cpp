// Stand-alone check of the index arithmetic that kernels of lb_kernels.h share (lodestar_amd/csrc/
// lb_kernel_index.h) for a sanitizer build (tests/test_kernel_index_cpu.py builds it with
// -fsanitize=address,undefined and -DLB_WT_MAX=<the kernels' value> and runs it):
//   * msm_for_digits<4> and <6>, the digit split of the bucket MSM's count and scatter passes, over
//     random 32-bit scalar halves times every weight 1 .. LB_WT_MAX: the digits recompose to the
//     product, a zero digit is never reported and no window index reaches W.  (<6> takes every
//     product, < 2^43; <4> serves weight 1 only, so its halves are drawn below 2^32 / weight.)
//   * seg_is_head / seg_next_head, the segment heads of a set's chunks [c0, c1): for every
//     c0 <= c1 <= 200 the walk from c0 visits exactly {c0} and the multiples of 64 in (c0, c1), and
//     seg_is_head names the same chunks.
// CPU only.
#include <stdio.h>

#include <vector>

#include "lb_kernel_index.h"

#ifndef LB_WT_MAX
#error "build with -DLB_WT_MAX=<the value of lb_kernels.h>"
#endif

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      failures++;                                                       \
      printf("kernel_index_check: FAILED line %d: %s\n", __LINE__, #c); \
    }                                                                   \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

template <int W, class K>
static void check_digits(K k) {
  uint64_t sum = 0;
  uint32_t seen = 0;
  int calls = 0;
  msm_for_digits<W>(k, [&](int w, uint32_t d) {
    calls++;
    CHECK(w >= 0 && w < W);
    CHECK(d != 0 && d < (uint32_t)LB_MSM_B);
    CHECK(!(seen & (1u << w)));  // each window at most once
    seen |= 1u << w;
    if (w >= 0 && w < W) sum += (uint64_t)d << (LB_MSM_C * w);
  });
  CHECK(sum == (uint64_t)k);
  int nonzero = 0;
  for (int w = 0; w < W; w++) nonzero += ((k >> (LB_MSM_C * w)) & (LB_MSM_B - 1)) != 0;
  CHECK(calls == nonzero);
}

static void check_msm_digits() {
  static_assert(LB_MSM_C * 6 >= 32 + 11 && (uint64_t)LB_WT_MAX < (1ull << 11), "six windows hold a weighted half");
  const uint32_t edge[] = {0u, 1u, 0xffu, 0x100u, 0xff00ff00u, 0x00ff00ffu, 0x80000000u, 0xffffffffu};
  for (uint32_t wt = 1; wt <= LB_WT_MAX; wt++) {
    for (int r = 0; r < 24; r++) {
      const uint32_t h = r < 8 ? edge[r] : rng32();
      check_digits<6>((uint64_t)h * wt);
      check_digits<4>((uint64_t)(h / wt) * wt);  // < 2^32
      check_digits<4>((h / wt) * wt);            // ... as the 32-bit value the weight-1 kernels pass
    }
  }
  for (int r = 0; r < 100000; r++) check_digits<4>(rng32());
}

static void check_segment_heads() {
  for (uint32_t c1 = 0; c1 <= 200; c1++) {
    for (uint32_t c0 = 0; c0 <= c1; c0++) {
      std::vector<uint32_t> want, walk, flagged;
      for (uint32_t c = c0; c < c1; c++) {
        if (c == c0 || c % 64 == 0) want.push_back(c);
        if (seg_is_head(c, c0)) flagged.push_back(c);
      }
      for (uint32_t c = c0; c < c1; c = seg_next_head(c)) walk.push_back(c);
      CHECK(walk == want);
      CHECK(flagged == want);
    }
  }
}

int main() {
  check_msm_digits();
  check_segment_heads();
  printf("kernel_index_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
