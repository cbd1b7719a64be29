// FK20: all 128 cell proofs of a blob (EIP-7594 computeCellsAndKzgProofs) from ONE pass over the
// setup instead of one 4096-term combination per cell.  LB_HD like lb_fr.h: the same source runs in
// the gfx950 kernels (lb_kzg_fk20.h), in lb_kzg_host.hip's host code (the twiddle table) and in the CPU
// harness (tests/harness/lb_kzg_fk20_harness.cpp).
//
// With a[0 .. 4095] the coefficients, s[t] = [tau^t] G1 and y_i = h_i^64 = w128^brp7(i), w128 = w^64:
//   proof_i = sum_{j < 63} y_i^j H_j,   H_j = sum_{u <= 4095 - 64 (j + 1)} a[u + 64 (j + 1)] s[u]
// so the proofs are the 128-point transform over w128 of (H_0 .. H_62, O, ..., O); natural-order
// output m is the proof of cell brp7(m).  The H_j are a Toeplitz product, taken by circulant
// embedding of size 128 for each residue i < 64 (fk_setup_index, fk_col_index):
//   x_i[j] = s[4031 - i - 64 j] (j < 63), else O;     X_i = DFT128(x_i)   the resident table
//   c_i[0] = a[4095 - i], c_i[1 .. 65] = 0, c_i[k] = a[64 (k - 64) - i - 1];  C_i = DFT128(c_i)
//   E[r] = sum_i C_i[r] X_i[r];   h = IDFT128(E);   h[0 .. 62] = H_j, h[63] = O
// h[64 .. 127] are NOT O: the forward transform reads its first 64 inputs only.
#pragma once
#include "lb_curve.h"
#include "lb_fr.h"

#define LB_FK_N 128u    // points per transform = CELLS_PER_EXT_BLOB
#define LB_FK_LOG 7
#define LB_FK_COLS 64u  // residues i: the stride of the Toeplitz product = FIELD_ELEMENTS_PER_CELL
#define LB_FK_POINTS (LB_FK_COLS * LB_FK_N)  // entries of the table X_i[r], entry 64 r + i
#define LB_FK_LIVE 64u  // inputs the proofs' forward transform reads
#define LB_FK_NONE 0xffffffffu
// the resident twiddle table (fk_tables), in entries of one fr: ladder scalars as plain LE words,
// the scalar-field side in Montgomery form
#define LB_FK_TAB_FWD 0u          // w128^k, k < 64, plain
#define LB_FK_TAB_INV 64u         // w128^-k, k < 64, plain
#define LB_FK_TAB_SCALE 128u      // 1 / 128, plain
#define LB_FK_TAB_FWD_MONT 129u   // w128^k, k < 64
#define LB_FK_TAB_INV_MONT 193u   // w128^-k, k < 64
#define LB_FK_TAB_SCALE_MONT 257u // 1 / 128
#define LB_FK_TAB_LEN 258u

LB_HD void fk_tables(fr* tab) {
  fr w = fr_sqr(fr_root8192());  // the 4096th root; its 32nd power is w128
  for (int i = 0; i < 5; i++) w = fr_sqr(w);
  const fr wi = fr_inv(w), sc = fr_inv(fr_from_u32(LB_FK_N));
  tab[LB_FK_TAB_FWD_MONT] = tab[LB_FK_TAB_INV_MONT] = fr_one();
  for (uint32_t k = 1; k < 64; k++) {
    tab[LB_FK_TAB_FWD_MONT + k] = fr_mul(tab[LB_FK_TAB_FWD_MONT + k - 1], w);
    tab[LB_FK_TAB_INV_MONT + k] = fr_mul(tab[LB_FK_TAB_INV_MONT + k - 1], wi);
  }
  tab[LB_FK_TAB_SCALE_MONT] = sc;
  for (uint32_t k = 0; k < 64; k++) {
    tab[LB_FK_TAB_FWD + k] = fr_from_mont(tab[LB_FK_TAB_FWD_MONT + k]);
    tab[LB_FK_TAB_INV + k] = fr_from_mont(tab[LB_FK_TAB_INV_MONT + k]);
  }
  tab[LB_FK_TAB_SCALE] = fr_from_mont(sc);
}

// the setup point that is x_i[j], the coefficient that is c_i[k]; LB_FK_NONE for O / 0
LB_HD uint32_t fk_setup_index(uint32_t i, uint32_t j) { return j < 63u ? 4031u - i - 64u * j : LB_FK_NONE; }
LB_HD uint32_t fk_col_index(uint32_t i, uint32_t k) {
  if (k == 0) return 4095u - i;
  return k < 66u ? LB_FK_NONE : 64u * (k - 64u) - i - 1u;
}

// ------------------------------------------------------------------ the 128-point transform
// out[m] = sum_j in[j] w^(j m) over any element type with an addition and a product by a power of w
// (fr: fr_mul by a table entry; G1: a 256-bit ladder), 64 lanes, one butterfly per lane per stage:
//   input j is loaded into slot fk_fft_slot(j) = brp7(j) (the reversal is the load's);
//   stage s = 0 .. 6: lane b pairs slots lo = 2 m (b div m) + (b mod m) and lo + m, m = 2^s, with
//   twiddle w^k, k = (b mod m) 2^(6 - s); k == 0 skips the product (all of stage 0);
//   barrier between stages (the caller's); output m is slot m.
// `A`: ld(i), st(i, v), add(u, v), sub(u, v).  `mulw(v, k)` = w^k v for 0 < k < 64.  The inverse
// transform is the same with w^-k and a scaling by 1 / 128, wherever the caller puts that.
LB_HD uint32_t fk_fft_slot(uint32_t j) { return fr_bitrev(j, LB_FK_LOG); }
template <class A, class M>
LB_HD void fk_fft_stage(A& a, int s, const M& mulw, uint32_t b) {
  const uint32_t m = 1u << s, j = b & (m - 1u), lo = ((b >> s) << (s + 1)) + j, hi = lo + m, k = j << (LB_FK_LOG - 1 - s);
  auto v = a.ld(hi);
  if (k) v = mulw(v, k);
  const auto u = a.ld(lo);
  a.st(lo, a.add(u, v));
  a.st(hi, a.sub(u, v));
}

// [k] P for a scalar below 2^255 (8 little-endian words) and a Jacobian base, infinity included:
// jac_mul_u256 with the full addition of jac_mul_u64_jac
template <class F>
LB_NI jac<F> jac_mul_u255_jac(jac<F> p, const uint32_t* k) {
  jac<F> acc = jac_infinity<F>();
  for (int i = 254; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((k[i >> 5] >> (i & 31)) & 1u) acc = jac_add_i(acc, p);
  }
  return acc;
}

// ------------------------------------------------------------------ the scalar side, per blob
// Column i of one blob, 64 lanes (lane t < 64), `A` an fr accessor over 128 slots, `coef` the blob's
// 4096 Montgomery coefficients: fk_col_load puts c_i[k] into slot brp7(k) for k = t, t + 64; seven
// fr_ntt_stage(A, 7, s, tw, t, 64) with tw(k) = w128^k follow (barriers the caller's); fk_col_store
// writes C_i[r] / 128 (the inverse transform's scaling, folded in here where it is one field
// product) for r = t, t + 64 as plain LE words at out_le + (64 r + i) * 8: the ladder scalars in the
// table's order.
template <class A, class C>
LB_HD void fk_col_load(A& a, const C& coef, uint32_t i, uint32_t t) {
  LB_UNROLL for (uint32_t k = t; k < LB_FK_N; k += 64u) {
    const uint32_t idx = fk_col_index(i, k);
    a.st(fk_fft_slot(k), idx == LB_FK_NONE ? fr_zero() : coef.ld(idx));
  }
}
template <class A>
LB_HD void fk_col_store(const A& a, const fr& inv_n, uint32_t i, uint32_t t, uint32_t* out_le) {
  LB_UNROLL for (uint32_t r = t; r < LB_FK_N; r += 64u)
    fr_to_le_words(out_le + ((size_t)LB_FK_COLS * r + i) * 8, fr_mul(a.ld(r), inv_n));
}
