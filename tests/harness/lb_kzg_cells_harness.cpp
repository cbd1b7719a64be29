// CPU harness of the host and per-lane pieces of the cell calls (EIP-7594): the combiner and the
// commitment deduplication of lb_kzg_transcript.h (kzg_cell_dedup, kzg_cell_batch_r, the threaded
// kzg_cell_batch_rs), the phases of k_fr_coset_ntt4096, k_fr_cell_interp, k_fr_cell_sum and
// k_fr_cell_quotient (kzg_cells_lanes.h over lb_fr.h) and the status fold of k_kzg_check_cells
// (lb_fr.h kzg_cell_group_status), compiled as plain C++ for tests/test_kzg_cells_cpu.py.  Field
// elements cross the boundary as 32 bytes: big endian where the wire has them so (cells, r), little
// endian plain form for coefficients and weights.  Test infrastructure only.
#include <string.h>
#include <vector>
#include "kzg_cells_lanes.h"
#include "lb_kzg_transcript.h"

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
static const fr* cell_tab() {
  static std::vector<fr> tab;
  if (tab.empty()) {
    tab.resize(LB_FR_CELL_TAB_LEN);
    fr_cell_tables(tab.data());
  }
  return tab.data();
}

extern "C" {
// w = 7^((r - 1) / 8192) as 32 little-endian bytes
void c_fr_root8192(uint8_t* out32le) {
  uint32_t w[8];
  fr_to_le_words(w, fr_root8192());
  wr_words(out32le, w);
}
// one group: r as 32 BE bytes, ci[n], first[<= n]; returns the number of distinct commitments
uint32_t c_kzg_cell_batch_r(uint32_t n, const uint8_t* commitments48, const uint32_t* cell_indices, const uint8_t* cells,
                            const uint8_t* proofs48, uint8_t* r32be, uint32_t* ci, uint32_t* first) {
  std::vector<uint32_t> f, c(n ? n : 1);
  const uint32_t nd = kzg_cell_dedup(n, commitments48, c.data(), f);
  for (uint32_t k = 0; k < n; k++) ci[k] = c[k];
  for (uint32_t d = 0; d < nd; d++) first[d] = f[d];
  kzg_fr_to_be32(r32be, kzg_cell_batch_r(n, commitments48, c.data(), f.data(), nd, cell_indices, cells, proofs48));
  return nd;
}
// many groups over flat arrays on `threads` threads: r_g as 32 BE bytes each
void c_kzg_cell_batch_rs(uint32_t n_groups, const uint32_t* off, const uint8_t* commitments48, const uint32_t* cell_indices,
                         const uint8_t* cells, const uint8_t* proofs48, uint32_t threads, uint8_t* r32be) {
  const uint32_t nc = off[n_groups];
  std::vector<uint32_t> ci(nc ? nc : 1), first, doff(n_groups + 1, 0);
  for (uint32_t g = 0; g < n_groups; g++)
    doff[g + 1] = doff[g] + kzg_cell_dedup(off[g + 1] - off[g], commitments48 + (size_t)48 * off[g], ci.data() + off[g], first);
  std::vector<fr> r(n_groups ? n_groups : 1);
  kzg_cell_batch_rs(n_groups, off, doff.data(), commitments48, ci.data(), first.data(), cell_indices, cells, proofs48, r.data(),
                    threads);
  for (uint32_t g = 0; g < n_groups; g++) kzg_fr_to_be32(r32be + 32 * g, r[g]);
}
// 4096 coefficients (LE) -> the 4096 values of cells 64 .. 127 as big-endian bytes
void c_fr_coset_ntt4096(const uint8_t* coeffs, uint8_t* out_cells_upper) {
  std::vector<fr> a(4096);
  for (uint32_t i = 0; i < 4096; i++) a[i] = rd_le(coeffs + 32 * i);
  std::vector<uint32_t> out((size_t)8 * 4096);
  coset_ntt4096_lanes(a.data(), cell_tab(), out.data());
  memcpy(out_cells_upper, out.data(), (size_t)32 * 4096);
}
// n_cells cells (2048 BE bytes each; returns how many hold an element >= r) with their indices and
// weights (LE) -> the weighted interpolation coefficients (n_cells x 64, LE) and the NEGATED sums of
// the groups off[g] .. off[g + 1] - 1 (n_groups x 64, LE)
uint32_t c_fr_cell_interp_sum(uint32_t n_groups, const uint32_t* off, uint32_t n_cells, const uint8_t* cells,
                              const uint32_t* cell_indices, const uint8_t* weights, uint8_t* out_coeffs, uint8_t* out_sums) {
  std::vector<fr> v((size_t)n_cells * 64 + 1), wt(n_cells + 1);
  uint32_t bad = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    bool ok = true;
    for (uint32_t t = 0; t < 64; t++) ok &= fr_from_be32(v[(size_t)c * 64 + t], cells + ((size_t)c * 64 + t) * 32);
    bad += ok ? 0 : 1;
    wt[c] = rd_le(weights + 32 * c);
  }
  cell_interp_lanes(n_cells, v.data(), cell_indices, wt.data(), cell_tab());
  for (size_t i = 0; i < (size_t)n_cells * 64; i++) {
    uint32_t w[8];
    fr_to_le_words(w, v[i]);
    wr_words(out_coeffs + 32 * i, w);
  }
  std::vector<uint32_t> sums((size_t)n_groups * 64 * 8 + 8);
  cell_sum_lanes(n_groups, off, n_cells, v.data(), sums.data());
  for (size_t i = 0; i < (size_t)n_groups * 64; i++) wr_words(out_sums + 32 * i, &sums[8 * i]);
  return bad;
}
// 4096 coefficients (LE) and a cell index -> the quotient's 4096 LE scalars
void c_fr_cell_quotient(const uint8_t* coeffs, uint32_t cell_index, uint8_t* q32) {
  std::vector<fr> a(4096);
  for (uint32_t i = 0; i < 4096; i++) a[i] = rd_le(coeffs + 32 * i);
  std::vector<uint32_t> q((size_t)8 * 4096, 0xAAAAAAAAu);
  cell_quotient_lanes(a.data(), cell_index, cell_tab(), q.data());
  for (uint32_t i = 0; i < 4096; i++) wr_words(q32 + 32 * i, &q[8 * i]);
}
int32_t c_kzg_cell_group_status(const int32_t* dstatus, uint32_t dlo, uint32_t dhi, const int32_t* cstatus, const int32_t* pstatus,
                                uint32_t lo, uint32_t hi) {
  return kzg_cell_group_status(dstatus, dlo, dhi, cstatus, pstatus, lo, hi);
}
}
