// CPU harness of the recovery pieces of lb_kzg_recover_cells_and_proofs (lb_recover.h through
// kzg_recover_lanes.h, and the argument check of lb_kzg_host.h), compiled as plain C++ for
// tests/test_kzg_recover_cpu.py.  Field elements cross the boundary as 32 little-endian bytes in plain
// form.  Test infrastructure only.
#include <string.h>
#include <vector>
#include "kzg_recover_lanes.h"
#include "lb_kzg_host.h"

static fr rd_le(const uint8_t* b) { return fr_to_mont(kzg_fr_from_le32(b)); }
static void wr_le(uint8_t* b, const fr& a) {
  uint32_t w[8];
  fr_to_le_words(w, a);
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) b[4 * k + s] = (uint8_t)(w[k] >> (8 * s));
}
struct rc_tabs {
  std::vector<fr> fk, cell;
  rc_tabs() : fk(LB_FK_TAB_LEN), cell(LB_FR_CELL_TAB_LEN) {
    fk_tables(fk.data());
    fr_cell_tables(cell.data());
  }
};
static const rc_tabs& tabs() {
  static const rc_tabs t;
  return t;
}

extern "C" {
uint32_t c_rc_point(uint32_t cell) { return rc_point(cell); }
uint32_t c_rc_slot(uint32_t cell) { return rc_slot(cell); }
uint32_t c_rc_rank(const uint32_t* mask, uint32_t cell) { return rc_rank(mask, cell); }
uint32_t c_rc_coef_index(uint32_t k, uint32_t r) { return rc_coef_index(k, r); }
// lb_kzg_recover_cells_and_proofs' argument check; mask: 4 n words
int c_rc_plan(uint32_t n, const uint32_t* off, const uint32_t* idx, uint32_t* mask) {
  memset(mask, 0, (size_t)16 * n);
  return kzg_recover_plan(n, off, idx, mask) ? 1 : 0;
}
// one blob's mask -> Zev and 1 / Zc, 128 values each
void c_rc_zero(const uint32_t* mask, uint8_t* zev_out, uint8_t* zcinv_out) {
  fr zev[LB_FK_N], zcinv[LB_FK_N];
  rc_zero_lanes(mask, tabs().fk.data(), tabs().cell.data(), zev, zcinv);
  for (uint32_t m = 0; m < LB_FK_N; m++) {
    wr_le(zev_out + 32 * m, zev[m]);
    wr_le(zcinv_out + 32 * m, zcinv[m]);
  }
}
// one blob: n_cells interpolated cells (64 coefficients each) with their indices -> the 4096
// coefficients, every column's upper half (64 x 64 values) and inconsistency flag (64).  -1 if the
// argument check rejects the indices.
int c_rc_recover(uint32_t n_cells, const uint32_t* idx, const uint8_t* interp, uint8_t* coef_out, uint8_t* upper_out, int32_t* flags) {
  const uint32_t off[2] = {0, n_cells};
  uint32_t mask[LB_RC_MASK_WORDS] = {0, 0, 0, 0};
  if (!kzg_recover_plan(1, off, idx, mask)) return -1;
  std::vector<fr> cells((size_t)n_cells * 64), coef(4096), upper(64);
  for (size_t i = 0; i < cells.size(); i++) cells[i] = rd_le(interp + 32 * i);
  fr zev[LB_FK_N], zcinv[LB_FK_N];
  rc_zero_lanes(mask, tabs().fk.data(), tabs().cell.data(), zev, zcinv);
  for (uint32_t r = 0; r < 64; r++) {
    flags[r] = rc_col_lanes(cells.data(), n_cells, 0, mask, zev, zcinv, tabs().fk.data(), tabs().cell.data(), r, coef.data(),
                            upper.data())
                   ? 1
                   : 0;
    for (uint32_t k = 0; k < 64; k++) wr_le(upper_out + 32 * (64 * r + k), upper[k]);
  }
  for (uint32_t j = 0; j < 4096; j++) wr_le(coef_out + 32 * j, coef[j]);
  return 0;
}
// 4096 coefficients -> the blob's 4096 elements by k_fr_ntt4096's schedule with nthr lanes
void c_rc_blob(const uint8_t* coef_in, uint32_t nthr, uint8_t* out) {
  std::vector<fr> coef(4096), v(4096);
  for (uint32_t j = 0; j < 4096; j++) coef[j] = rd_le(coef_in + 32 * j);
  rc_blob_lanes(coef.data(), tabs().cell.data(), nthr, v.data());
  for (uint32_t j = 0; j < 4096; j++) wr_le(out + 32 * j, v[j]);
}
}
