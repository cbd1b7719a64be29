// Cell recovery (EIP-7594 recoverCellsAndKzgProofs): the blob's 4096 monomial coefficients from any
// 64 .. 128 of its cells, as 64 independent erasure decodes of size 128.  LB_HD like lb_fr.h and
// lb_fk20.h: the same source runs in the gfx950 kernels (lb_kzg_field.h k_fr_recover_*) and in the
// CPU harness (tests/harness/lb_kzg_recover_harness.cpp).
//
// Write p(X) = sum_{r < 64} X^r P_r(X^64), deg P_r < 64.  On cell i the coset is h_i <w64> and X^64 is
// the constant y_i = h_i^64 = w128^brp7(i) (w128 = w^64), so coefficient r of the cell's
// interpolation polynomial (k_fr_cell_interp, unit weight) is P_r(y_i): every P_r is known at the
// points w128^m, m = brp7(i) = rc_point(i), of the given cells.  With
//   Z(Y) = prod over the missing cells of (Y - y_i)        (degree <= 64; 1 when nothing is missing)
// and a shift s with s^128 != 1 (s = w, the 8192nd root whose powers the cell table holds), column r is
//   E[m] = P_r(w128^m) at given cells, 0 at missing ones;   N = IDFT128(E Zev),  Zev[m] = Z(w128^m)
//   Q    = IDFT128( DFT128(N[k] s^k) / Zc ) [k] s^-k,       Zc[m] = Z(s w128^m)
// and Q[k], k < 64, is coefficient 64 k + r of p.  N = P_r Z has degree < 128, so nothing wraps.
// Q[64 .. 127] = 0 for every column exactly when the given cells lie on one polynomial of degree
// < 4096: then Q Z and N agree on 128 points with both of degree < 128, so Q = E at every given cell.
// With exactly 64 cells that always holds.  The two 1 / 128 of the inverse transforms are taken
// together at the end (rc_col_store).
#pragma once
#include "lb_fk20.h"

#define LB_RC_MASK_WORDS 4u   // the present-cell mask of one blob: bit (i mod 32) of word i div 32

// cell i's point is w128^rc_point(i); as an input of a transform it goes to slot
// fk_fft_slot(rc_point(i)), which is i again: the cells stand in the transform's own input order
LB_HD uint32_t rc_point(uint32_t cell) { return fr_bitrev(cell, LB_FK_LOG); }
LB_HD uint32_t rc_slot(uint32_t cell) { return fk_fft_slot(rc_point(cell)); }
// word w < 4 of a mask and the rank below are written without a variable index: in a kernel the
// mask's four words stay in registers
LB_HD uint32_t rc_mask_word(const uint32_t* mask, uint32_t w) {
  uint32_t v = 0;
  LB_UNROLL for (uint32_t k = 0; k < LB_RC_MASK_WORDS; k++) v = w == k ? mask[k] : v;
  return v;
}
LB_HD bool rc_present(const uint32_t* mask, uint32_t cell) { return (rc_mask_word(mask, cell >> 5) >> (cell & 31u)) & 1u; }
LB_HD uint32_t rc_popcount(uint32_t v) {
  v = v - ((v >> 1) & 0x55555555u);
  v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
  return (((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}
// the given cells below `cell`: where cell `cell` stands among its blob's given cells (ascending)
LB_HD uint32_t rc_rank(const uint32_t* mask, uint32_t cell) {
  const uint32_t cw = cell >> 5, below = (1u << (cell & 31u)) - 1u;
  uint32_t n = 0;
  LB_UNROLL for (uint32_t k = 0; k < LB_RC_MASK_WORDS; k++) n += rc_popcount(mask[k] & (k < cw ? 0xffffffffu : (k == cw ? below : 0u)));
  return n;
}
// w128^m for m < 128 from tw(k) = w128^k, k < 64 (fk_tables, Montgomery): w128^64 = -1
template <class T>
LB_HD fr rc_root(const T& tw, uint32_t m) {
  return m < 64u ? tw(m) : fr_neg(tw(m - 64u));
}

// ------------------------------------------------------------------ the vanishing polynomial, per blob
// Z(x) by its definition, one factor per missing cell
template <class T>
LB_HD fr rc_vanish_at(const uint32_t* mask, const T& tw, const fr& x) {
  fr acc = fr_one();
  for (uint32_t i = 0; i < LB_FK_N; i++)
    if (!rc_present(mask, i)) acc = fr_mul(acc, fr_sub(x, rc_root(tw, rc_point(i))));
  return acc;
}
// lane t < 64 of a blob's wave (k_fr_recover_zero): Zev[m] and 1 / Zc[m] for m = t, t + 64 (Montgomery,
// 8 words each at zev + 8 m, zcinv + 8 m).  s: the shift.  Zc[m] != 0: s w128^m is no 128th root of unity.
template <class T>
LB_HD void rc_zero_lane(const uint32_t* mask, const T& tw, const fr& s, uint32_t t, uint32_t* zev, uint32_t* zcinv) {
  for (uint32_t m = t; m < LB_FK_N; m += 64u) {
    const fr x = rc_root(tw, m);
    const fr a = rc_vanish_at(mask, tw, x), b = fr_inv(rc_vanish_at(mask, tw, fr_mul(s, x)));
    for (int w = 0; w < 8; w++) {
      zev[(size_t)8 * m + w] = a.l[w];
      zcinv[(size_t)8 * m + w] = b.l[w];
    }
  }
}

// ------------------------------------------------------------------ one column, 64 lanes
// `A`: 128 slots with ld / st / add / sub (fk_fft_stage's accessor); lane t < 64; barriers between the
// phases are the caller's:
//   rc_col_load;  7 x fk_fft_stage (w128^-k);                          N, unscaled
//   rc_take(sh);  barrier;  rc_put;  7 x fk_fft_stage (w128^k);        N(s w128^m)
//   rc_take(zcinv);  barrier;  rc_put;  7 x fk_fft_stage (w128^-k);    Q[k] s^k, unscaled
//   rc_col_store.
// cells(k, r): coefficient r of the k-th interpolated cell of the call, the blob's given cells being
// lo .. lo + count - 1 in ascending cell order; zev(m), zcinv(m): rc_zero_lane's values.
template <class A, class C, class Z>
LB_HD void rc_col_load(A& a, const C& cells, const uint32_t* mask, uint32_t lo, const Z& zev, uint32_t r, uint32_t t) {
  LB_UNROLL for (uint32_t i = t; i < LB_FK_N; i += 64u)
    a.st(rc_slot(i), rc_present(mask, i) ? fr_mul(cells(lo + rc_rank(mask, i), r), zev(rc_point(i))) : fr_zero());
}
// the natural-order outputs k = t, t + 64 of one transform times mul(k), and back in as the inputs of the next
template <class A, class M>
LB_HD void rc_take(const A& a, const M& mul, uint32_t t, fr v[2]) {
  LB_UNROLL for (uint32_t j = 0; j < 2u; j++) v[j] = fr_mul(a.ld(t + 64u * j), mul(t + 64u * j));
}
template <class A>
LB_HD void rc_put(A& a, uint32_t t, const fr v[2]) {
  LB_UNROLL for (uint32_t j = 0; j < 2u; j++) a.st(fk_fft_slot(t + 64u * j), v[j]);
}
// where Q[k] of column r goes among the blob's 4096 coefficients
LB_HD uint32_t rc_coef_index(uint32_t k, uint32_t r) { return 64u * k + r; }
// Q[t] s^-t / 128^2 -> coef (8 Montgomery words per coefficient); true if Q[t + 64] != 0: the given
// cells lie on no polynomial of degree < 4096 (the scalings cannot make a zero of it or undo one)
template <class A, class M>
LB_HD bool rc_col_store(const A& a, const M& shinv, const fr& inv_n2, uint32_t r, uint32_t t, uint32_t* coef) {
  const fr q = fr_mul(fr_mul(a.ld(t), shinv(t)), inv_n2);
  for (int w = 0; w < 8; w++) coef[(size_t)8 * rc_coef_index(t, r) + w] = q.l[w];
  return !fr_is_zero(a.ld(t + 64u));
}

// ------------------------------------------------------------------ the blob's bytes from its coefficients
// k_fr_ntt4096: coefficient j goes to slot brp12(j) (the transform's input reversal done by the load,
// as in fr_coset_load but unscaled), twelve forward fr_ntt_stage with tw(k) = w^(2 k) follow, and
// fr_coset_value(a, k) is p at the blob's k-th bit-reversed root: element k of the blob.
template <class A, class C>
LB_HD void rc_blob_load(A& a, const C& coef, uint32_t tid, uint32_t nthr) {
  for (uint32_t j = tid; j < 4096u; j += nthr) a.st(fr_bitrev(j, 12), coef.ld(j));
}
