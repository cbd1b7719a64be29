// The phases of the cell kernels (lb_kzg_field.h k_fr_coset_ntt4096, k_fr_cell_interp, k_fr_cell_sum,
// k_fr_cell_quotient) on the CPU: the same lb_fr.h lane functions, the workgroup's lanes in turn
// where the kernel has a barrier, exactly the kernels' addressing.  `tab` is fr_cell_tables' table.
// Shared by tests/harness/lb_kzg_cells_harness.cpp and tests/native/kzg_cells_check.cpp.
#pragma once
#include <vector>
#include "lb_fr.h"
#include "fr_views.h"

struct kzg_cells_of {
  const fr* p;
  fr operator()(uint32_t k, uint32_t j) const { return p[(size_t)k * LB_FR_CELL + j]; }
};

// k_fr_coset_ntt4096 for one blob, 1024 lanes: out_be = the 4096 values of cells 64 .. 127 as words
// whose little-endian storage is the big-endian bytes
static inline void coset_ntt4096_lanes(const fr* coef, const fr* tab, uint32_t* out_be) {
  const uint32_t lanes = 1024;
  std::vector<fr> lds(4096);
  fr_view A{lds.data()};
  const fr_cview C{coef};
  const fr_table SC{tab + LB_FR_CELL_TAB_SCALE}, T{tab + LB_FR_CELL_TAB_FWD};
  for (uint32_t t = 0; t < lanes; t++) fr_coset_load(A, C, SC, t, lanes);
  for (int s = 0; s < 12; s++)
    for (uint32_t t = 0; t < lanes; t++) fr_ntt_stage(A, 12, s, T, t, lanes);
  for (uint32_t t = 0; t < lanes; t++)
    for (uint32_t k = t; k < 4096; k += lanes) fr_to_be_words(out_be + (size_t)8 * k, fr_coset_value(A, k));
}

// k_fr_cell_interp over n_cells cells in place (one wave of 64 lanes each)
static inline void cell_interp_lanes(uint32_t n_cells, fr* cells, const uint32_t* cell_index, const fr* weight, const fr* tab) {
  const fr_table T{tab + LB_FR_CELL_TAB_ITW}, W{tab + LB_FR_CELL_TAB_WINV};
  for (uint32_t c = 0; c < n_cells; c++) {
    fr lds[LB_FR_CELL];
    fr_view V{lds};
    for (uint32_t t = 0; t < LB_FR_CELL; t++) V.st(t, cells[(size_t)c * LB_FR_CELL + t]);
    for (int s = 0; s < LB_FR_CELL_LOG; s++)
      for (uint32_t t = 0; t < LB_FR_CELL; t++) fr_ntt_stage(V, LB_FR_CELL_LOG, s, T, t, LB_FR_CELL);
    for (uint32_t t = 0; t < LB_FR_CELL; t++)
      cells[(size_t)c * LB_FR_CELL + t] =
          fr_cell_descale(V.ld(t), T(LB_FR_CELL / 2), W, cell_index[c] & (LB_FR_CELLS - 1u), t, weight[c]);
  }
}

// k_fr_cell_sum: the negated per-group sums as plain LE words at out_le + (64 g + j) * 8
static inline void cell_sum_lanes(uint32_t n_groups, const uint32_t* off, uint32_t n_cells, const fr* cells, uint32_t* out_le) {
  for (uint32_t g = 0; g < n_groups; g++) {
    const uint32_t hi = off[g + 1] < n_cells ? off[g + 1] : n_cells, lo = off[g] < hi ? off[g] : hi;
    for (uint32_t j = 0; j < LB_FR_CELL; j++)
      fr_to_le_words(out_le + ((size_t)g * LB_FR_CELL + j) * 8, fr_neg(fr_cell_group_sum(kzg_cells_of{cells}, lo, hi, j)));
  }
}

// k_fr_cell_quotient for one (blob, cell): 4096 plain LE scalars
static inline void cell_quotient_lanes(const fr* coef, uint32_t cell_index, const fr* tab, uint32_t* q_le) {
  const fr_table W{tab + LB_FR_CELL_TAB_WINV};
  for (uint32_t l = 0; l < 64; l++)
    fr_cell_quotient_lane(fr_cview{coef}, 4096u, W(fr_cell_h64_index(cell_index & (LB_FR_CELLS - 1u))), l, q_le);
}
