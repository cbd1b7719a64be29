// CPU harness of the FK20 pieces of lb_kzg_compute_cells_and_proofs (lb_fk20.h): the column gather
// and transforms of k_fr_fk_cols and the stage schedule of k_g1_fft128, over fr and over G1 points
// (kzg_fk20_lanes.h), compiled as plain C++ for tests/test_kzg_fk20_cpu.py.  Field elements cross the
// boundary as 32 little-endian bytes in plain form, points as x || y (48 big-endian bytes each) with
// a flag for infinity.  Test infrastructure only.
#include <string.h>
#include <vector>
#include "kzg_fk20_lanes.h"
#include "lb_serial.h"

static fr rd_le(const uint8_t* b) {
  fr p;
  for (int w = 0; w < 8; w++)
    p.l[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
  return fr_to_mont(p);
}
static void wr_words(uint8_t* b, const uint32_t* w) {
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) b[4 * k + s] = (uint8_t)(w[k] >> (8 * s));
}
static const fr* fk_tab() {
  static std::vector<fr> tab;
  if (tab.empty()) {
    tab.resize(LB_FK_TAB_LEN);
    fk_tables(tab.data());
  }
  return tab.data();
}

extern "C" {
// 4096 coefficients (LE) -> the 8192 ladder scalars (LE), scalar 64 r + i = C_i[r] / 128
void c_fk_cols(const uint8_t* coeffs, uint8_t* out) {
  std::vector<fr> a(4096);
  for (uint32_t i = 0; i < 4096; i++) a[i] = rd_le(coeffs + 32 * i);
  std::vector<uint32_t> le((size_t)8 * LB_FK_POINTS, 0xAAAAAAAAu);
  fk_cols_lanes(a.data(), fk_tab(), le.data());
  for (uint32_t i = 0; i < LB_FK_POINTS; i++) wr_words(out + 32 * i, &le[8 * i]);
}
// the transform's schedule over fr: 128 values (LE) -> 128 values (LE)
void c_fk_fft_fr(const uint8_t* in, uint32_t n_live, int inverse, int scale, uint8_t* out) {
  fr a[LB_FK_N], o[LB_FK_N];
  for (uint32_t i = 0; i < LB_FK_N; i++) a[i] = rd_le(in + 32 * i);
  fk_fft_fr_lanes(a, n_live, fk_tab(), inverse != 0, scale != 0, o);
  for (uint32_t i = 0; i < LB_FK_N; i++) {
    uint32_t w[8];
    fr_to_le_words(w, o[i]);
    wr_words(out + 32 * i, w);
  }
}
// ... over G1: input j = [k[j]] G (k[j] = 0: infinity); output m as x || y at out96 + 96 m, inf[m] = 1
// for infinity
void c_fk_fft_g1(const uint64_t* k, uint32_t n_live, int inverse, int scale, uint8_t* out96, int32_t* inf) {
  const g1a g{fp_load(LB_G1X), fp_load(LB_G1Y)};
  std::vector<g1j> a(LB_FK_N), o(LB_FK_N);
  for (uint32_t j = 0; j < LB_FK_N; j++) a[j] = k[j] ? jac_mul_u64(g, k[j]) : jac_infinity<fp>();
  fk_fft_g1_lanes(a.data(), n_live, fk_tab(), inverse != 0, scale != 0, o.data());
  for (uint32_t m = 0; m < LB_FK_N; m++) {
    g1a p;
    inf[m] = jac_to_aff(p, o[m]) ? 0 : 1;
    fp_plain_to_be48(out96 + 96 * m, fp_from_mont(p.x));
    fp_plain_to_be48(out96 + 96 * m + 48, fp_from_mont(p.y));
  }
}
// the index maps, for the table's layout
uint32_t c_fk_setup_index(uint32_t i, uint32_t j) { return fk_setup_index(i, j); }
uint32_t c_fk_col_index(uint32_t i, uint32_t k) { return fk_col_index(i, k); }
}
