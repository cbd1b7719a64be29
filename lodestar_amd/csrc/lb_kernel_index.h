// Index arithmetic of lb_kernels.h that more than one kernel has to agree on, free of device code
// so that a CPU program can call it (tests/native/kernel_index_check.cpp).
#pragma once
#include "lb_common.h"

// ---- segment heads (lb_kernels.h wave_segments, wave_seg_sum)
// The chunk sums of one set (or of one root) are combined by a segmented shuffle tree over the wave
// that computed them, chunk c on lane c % LB_WAVE.  The tree leaves each segment's sum on the
// segment's first lane, so the set's sum is the sum of its segment heads: its first chunk c0 and
// every later chunk on a wave's first lane.  A reader walks c0, seg_next_head(c0), ... below its end.
#define LB_WAVE 64u  // lanes of a wave
LB_HD bool seg_is_head(uint32_t c, uint32_t c0) { return c == c0 || (c & (LB_WAVE - 1)) == 0; }
LB_HD uint32_t seg_next_head(uint32_t c) { return (c / LB_WAVE + 1) * LB_WAVE; }

// ---- digits of the bucket MSM (lb_kernels.h k_msm_*, k_smsm_*)
// Pippenger windows of LB_MSM_C bits: a point whose scalar half k has the non-zero digit d in
// window w joins bucket (w, d).  msm_for_digits calls f(w, d) for each of them, w < W; the count
// and the scatter pass of one MSM must enumerate the same digits, and k < 2^(LB_MSM_C W).  K: uint32_t
// (a scalar half by itself) or uint64_t (a half times a weight), so neither pays for the other's width.
#define LB_MSM_C 8
#define LB_MSM_B (1 << LB_MSM_C)
template <int W, class K, class Fn>
LB_HD void msm_for_digits(K k, Fn f) {
  LB_UNROLL for (int w = 0; w < W; w++) {
    const uint32_t d = (uint32_t)(k >> (LB_MSM_C * w)) & (LB_MSM_B - 1);
    if (d) f(w, d);
  }
}
