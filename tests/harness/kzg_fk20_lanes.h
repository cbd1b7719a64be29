// The phases of the FK20 kernels (lb_kzg_fk20.h k_g1_fft128, k_fr_fk_cols) on the CPU: the same
// lb_fk20.h lane functions, the wave's 64 lanes in turn where the kernel has a barrier, exactly the
// kernels' addressing.  The transform's schedule runs over fr (checked against a plain recursive
// transform) and over G1 points.  `tab` is fk_tables' table.  Shared by
// tests/harness/lb_kzg_fk20_harness.cpp and tests/native/kzg_fk20_check.cpp.
#pragma once
#include <vector>
#include "lb_fk20.h"
#include "fr_views.h"

struct fk_fr_slots {
  fr* p;
  fr ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const fr& v) { p[i] = v; }
  fr add(const fr& u, const fr& v) const { return fr_add(u, v); }
  fr sub(const fr& u, const fr& v) const { return fr_sub(u, v); }
};
struct fk_fr_mulw {
  const fr* tw;  // Montgomery
  fr operator()(const fr& v, uint32_t k) const { return fr_mul(v, tw[k]); }
};
struct fk_g1_slots {
  g1j* p;
  g1j ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const g1j& v) { p[i] = v; }
  g1j add(const g1j& u, const g1j& v) const { return jac_add_i(u, v); }
  g1j sub(const g1j& u, const g1j& v) const { return jac_add_i(u, jac_neg(v)); }
};
struct fk_g1_mulw_cpu {
  const fr* tw;  // plain LE words
  g1j operator()(const g1j& v, uint32_t k) const { return jac_mul_u255_jac(v, tw[k].l); }
};

// the schedule of k_g1_fft128 over fr: inputs from n_live on are 0
static inline void fk_fft_fr_lanes(const fr* in, uint32_t n_live, const fr* tab, bool inverse, bool scale, fr* out) {
  fr lds[LB_FK_N];
  fk_fr_slots A{lds};
  const fk_fr_mulw M{tab + (inverse ? LB_FK_TAB_INV_MONT : LB_FK_TAB_FWD_MONT)};
  for (uint32_t lane = 0; lane < 64; lane++)
    for (uint32_t j = lane; j < LB_FK_N; j += 64) A.st(fk_fft_slot(j), j < n_live ? in[j] : fr_zero());
  for (int s = 0; s < LB_FK_LOG; s++)
    for (uint32_t lane = 0; lane < 64; lane++) fk_fft_stage(A, s, M, lane);
  for (uint32_t m = 0; m < LB_FK_N; m++) out[m] = scale ? fr_mul(A.ld(m), tab[LB_FK_TAB_SCALE_MONT]) : A.ld(m);
}

// k_g1_fft128 for one transform
static inline void fk_fft_g1_lanes(const g1j* in, uint32_t n_live, const fr* tab, bool inverse, bool scale, g1j* out) {
  std::vector<g1j> lds(LB_FK_N);
  fk_g1_slots A{lds.data()};
  const fk_g1_mulw_cpu M{tab + (inverse ? LB_FK_TAB_INV : LB_FK_TAB_FWD)};
  for (uint32_t lane = 0; lane < 64; lane++)
    for (uint32_t j = lane; j < LB_FK_N; j += 64) A.st(fk_fft_slot(j), j < n_live ? in[j] : jac_infinity<fp>());
  for (int s = 0; s < LB_FK_LOG; s++)
    for (uint32_t lane = 0; lane < 64; lane++) fk_fft_stage(A, s, M, lane);
  for (uint32_t m = 0; m < LB_FK_N; m++) out[m] = scale ? jac_mul_u255_jac(A.ld(m), tab[LB_FK_TAB_SCALE].l) : A.ld(m);
}

// k_fr_fk_cols for one blob: 8192 plain LE scalars, scalar 64 r + i = C_i[r] / 128
static inline void fk_cols_lanes(const fr* coef, const fr* tab, uint32_t* out_le) {
  const fr_table T{tab + LB_FK_TAB_FWD_MONT};
  for (uint32_t i = 0; i < LB_FK_COLS; i++) {
    fr lds[LB_FK_N];
    fk_fr_slots V{lds};
    for (uint32_t t = 0; t < 64; t++) fk_col_load(V, fr_cview{coef}, i, t);
    for (int s = 0; s < LB_FK_LOG; s++)
      for (uint32_t t = 0; t < 64; t++) fr_ntt_stage(V, LB_FK_LOG, s, T, t, 64u);
    for (uint32_t t = 0; t < 64; t++) fk_col_store(V, tab[LB_FK_TAB_SCALE_MONT], i, t, out_le);
  }
}
