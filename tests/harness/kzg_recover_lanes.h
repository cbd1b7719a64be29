// The phases of the recovery kernels (lb_kzg_field.h k_fr_recover_zero, k_fr_recover_cols, k_fr_ntt4096)
// on the CPU: the same lb_recover.h lane functions, the wave's 64 lanes in turn where the kernel has
// a barrier, exactly the kernels' addressing.  `fk` is fk_tables' table, `tab` fr_cell_tables'.  Shared
// by tests/harness/lb_kzg_recover_harness.cpp and tests/native/kzg_recover_check.cpp.
#pragma once
#include <vector>
#include "lb_recover.h"
#include "kzg_fk20_lanes.h"

// the interpolated cells of one call: coefficient j of cell k at p[64 k + j]
struct rc_cells_view {
  const fr* p;
  uint32_t n_cells;
  fr operator()(uint32_t k, uint32_t j) const { return p[(size_t)(k < n_cells ? k : n_cells - 1) * 64 + j]; }
};

// k_fr_recover_zero for one blob: zev, zcinv as 128 Montgomery values each
static inline void rc_zero_lanes(const uint32_t* mask, const fr* fk, const fr* tab, fr* zev, fr* zcinv) {
  for (uint32_t t = 0; t < 64; t++)
    rc_zero_lane(mask, fr_table{fk + LB_FK_TAB_FWD_MONT}, tab[LB_FR_CELL_TAB_SCALE + 1], t, reinterpret_cast<uint32_t*>(zev), reinterpret_cast<uint32_t*>(zcinv));
}

// k_fr_recover_cols for one (blob, column): writes the column's 64 coefficients into coef (4096
// values) and returns whether any lane saw a non-zero upper half; upper (if given) gets slots 64 .. 127
static inline bool rc_col_lanes(const fr* cells, uint32_t n_cells, uint32_t lo, const uint32_t* mask, const fr* zev, const fr* zcinv,
                                const fr* fk, const fr* tab, uint32_t r, fr* coef, fr* upper) {
  fr lds[LB_FK_N], v[64][2];
  fk_fr_slots V{lds};
  const fk_fr_mulw FW{fk + LB_FK_TAB_FWD_MONT}, IW{fk + LB_FK_TAB_INV_MONT};
  for (uint32_t t = 0; t < 64; t++) rc_col_load(V, rc_cells_view{cells, n_cells}, mask, lo, fr_table{zev}, r, t);
  for (int s = 0; s < LB_FK_LOG; s++)
    for (uint32_t t = 0; t < 64; t++) fk_fft_stage(V, s, IW, t);
  for (uint32_t t = 0; t < 64; t++) rc_take(V, fr_table{tab + LB_FR_CELL_TAB_SCALE}, t, v[t]);
  for (uint32_t t = 0; t < 64; t++) rc_put(V, t, v[t]);
  for (int s = 0; s < LB_FK_LOG; s++)
    for (uint32_t t = 0; t < 64; t++) fk_fft_stage(V, s, FW, t);
  for (uint32_t t = 0; t < 64; t++) rc_take(V, fr_table{zcinv}, t, v[t]);
  for (uint32_t t = 0; t < 64; t++) rc_put(V, t, v[t]);
  for (int s = 0; s < LB_FK_LOG; s++)
    for (uint32_t t = 0; t < 64; t++) fk_fft_stage(V, s, IW, t);
  bool bad = false;
  for (uint32_t t = 0; t < 64; t++)
    bad |= rc_col_store(V, fr_table{tab + LB_FR_CELL_TAB_WINV}, fr_sqr(fk[LB_FK_TAB_SCALE_MONT]), r, t, reinterpret_cast<uint32_t*>(coef));
  if (upper)
    for (uint32_t k = 0; k < 64; k++) upper[k] = V.ld(64 + k);
  return bad;
}

// k_fr_ntt4096 for one blob: 4096 coefficients -> the blob's 4096 elements (Montgomery), `nthr` lanes
static inline void rc_blob_lanes(const fr* coef, const fr* tab, uint32_t nthr, fr* out) {
  std::vector<fr> lds(4096);
  fr_view A{lds.data()};
  const fr_table T{tab + LB_FR_CELL_TAB_FWD};
  for (uint32_t t = 0; t < nthr; t++) rc_blob_load(A, fr_cview{coef}, t, nthr);
  for (int s = 0; s < 12; s++)
    for (uint32_t t = 0; t < nthr; t++) fr_ntt_stage(A, 12, s, T, t, nthr);
  for (uint32_t k = 0; k < 4096; k++) out[k] = fr_coset_value(A, k);
}
