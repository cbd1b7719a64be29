// The phases of k_fr_eval_quotient_many (lb_kzg_field.h) on the CPU, workgroup k and its lanes in
// turn: polynomial k (n coefficients, n / 4 a power of two) at its own point z[k], the quotient's
// n plain LE scalars at q_le + k * n * 8 and y_k at y_le + 8 k, exactly the kernel's addressing.
// Shared by tests/harness/lb_kzg_blob_harness.cpp and tests/native/kzg_blob_check.cpp.
#pragma once
#include <vector>
#include "lb_fr.h"
#include "fr_views.h"

static inline void eval_quotient_many_lanes(uint32_t n_polys, uint32_t n, const fr* coef, const fr* z_all, uint32_t* q_le,
                                            uint32_t* y_le) {
  const uint32_t lanes = n / 4;
  std::vector<fr> buf0(lanes), buf1(lanes);
  for (uint32_t k = 0; k < n_polys; k++) {
    const fr_cview A{coef + (size_t)k * n};
    const fr z = z_all[k];
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
    for (uint32_t t = 0; t < lanes; t++) fr_eq_finish(A, z, src, lanes, t, q_le + (size_t)k * n * 8, y_le + (size_t)8 * k);
  }
}
