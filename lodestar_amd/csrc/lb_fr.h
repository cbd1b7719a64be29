// The BLS12-381 scalar field Fr (r = 0x73eda753 299d7d48 3339d808 09a1d805 53bda402 fffe5bfe
// ffffffff 00000001, the G1 subgroup order): the field of KZG blob elements, polynomial
// coefficients and Fiat-Shamir challenges.  LB_HD like the rest of the arithmetic, so the same
// source runs in the gfx950 kernels (lb_kzg_field.h), in lb_kzg_host.hip's host code (twiddle
// table, challenges) and in the CPU harness (tests/harness/lb_fr_harness.cpp).
//
// Representation: Montgomery form with R = 2^256, eight 32-bit limbs, little endian.  Products are
// CIOS over (uint64_t)a * b + c + d, which the device compiles to v_mad_u64_u32.  r < 2^255, so
// a product of two values below r is below 2 r before its one conditional subtraction.
//
// The transform (fr_ntt_*) and the evaluate-and-divide scan (fr_eq_*) are written per lane over
// an accessor, with the barriers left to the caller: a kernel runs one call per thread between
// __syncthreads(), the CPU harness loops over the lanes between the phases.
#pragma once
#include "lb_common.h"

struct fr {
  uint32_t l[8];
};

#define LB_FR_MOD_WORDS \
  { 0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u }
// 2^256 mod r (Montgomery one) and 2^512 mod r
#define LB_FR_ONE_WORDS \
  { 0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u }
#define LB_FR_R2_WORDS \
  { 0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u }
// 7^((r - 1) / 4096): the primitive 4096th root of unity of the blob domain (plain form)
#define LB_FR_ROOT4096_WORDS \
  { 0xa5d36306u, 0xe206da11u, 0x378fbf96u, 0x0ad1347bu, 0xe0f8245fu, 0xfc3e8acfu, 0xa0f704f4u, 0x564c0a11u }
// -r^-1 mod 2^32 (r = 1 mod 2^32)
#define LB_FR_N0 0xffffffffu

LB_HD fr fr_zero() {
  fr z;
  LB_UNROLL for (int i = 0; i < 8; i++) z.l[i] = 0;
  return z;
}
LB_HD fr fr_from_words(const uint32_t w[8]) {
  fr a;
  LB_UNROLL for (int i = 0; i < 8; i++) a.l[i] = w[i];
  return a;
}
LB_HD fr fr_one() {
  const uint32_t w[8] = LB_FR_ONE_WORDS;
  return fr_from_words(w);
}
LB_HD bool fr_is_zero(const fr& a) {
  uint32_t o = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) o |= a.l[i];
  return o == 0;
}
LB_HD bool fr_eq(const fr& a, const fr& b) {
  uint32_t o = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) o |= a.l[i] ^ b.l[i];
  return o == 0;
}

// a - r if that is >= 0 (or `carry` says a stands for a + 2^256), else a
LB_HD fr fr_csub(const fr& a, uint32_t carry) {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  fr d;
  uint32_t bw = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) d.l[i] = LB_SUBC(a.l[i], m[i], bw, &bw);
  const bool take = carry != 0 || bw == 0;
  fr o;
  LB_UNROLL for (int i = 0; i < 8; i++) o.l[i] = take ? d.l[i] : a.l[i];
  return o;
}
// a plain 256-bit value below r?
LB_HD bool fr_lt_mod(const fr& a) {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  uint32_t bw = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) (void)LB_SUBC(a.l[i], m[i], bw, &bw);
  return bw != 0;
}

LB_HD fr fr_add(const fr& a, const fr& b) {
  fr s;
  uint32_t c = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) s.l[i] = LB_ADDC(a.l[i], b.l[i], c, &c);
  return fr_csub(s, c);  // a + b < 2 r < 2^256: c is 0, kept for inputs that are not reduced
}
LB_HD fr fr_sub(const fr& a, const fr& b) {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  fr d;
  uint32_t bw = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) d.l[i] = LB_SUBC(a.l[i], b.l[i], bw, &bw);
  const uint32_t mask = 0u - bw;
  uint32_t c = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) d.l[i] = LB_ADDC(d.l[i], m[i] & mask, c, &c);
  return d;
}
LB_HD fr fr_neg(const fr& a) { return fr_sub(fr_zero(), a); }

// Montgomery product a b / 2^256 mod r (CIOS, one 32-bit limb of b per round)
LB_HD fr fr_mul(const fr& a, const fr& b) {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  uint32_t t[10];
  LB_UNROLL for (int i = 0; i < 10; i++) t[i] = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) {
    uint64_t uv;
    uint32_t c = 0;
    LB_UNROLL for (int j = 0; j < 8; j++) {
      uv = (uint64_t)a.l[j] * b.l[i] + t[j] + c;
      t[j] = (uint32_t)uv;
      c = (uint32_t)(uv >> 32);
    }
    uv = (uint64_t)t[8] + c;
    t[8] = (uint32_t)uv;
    t[9] = (uint32_t)(uv >> 32);
    const uint32_t q = t[0] * LB_FR_N0;
    uv = (uint64_t)q * m[0] + t[0];
    c = (uint32_t)(uv >> 32);
    LB_UNROLL for (int j = 1; j < 8; j++) {
      uv = (uint64_t)q * m[j] + t[j] + c;
      t[j - 1] = (uint32_t)uv;
      c = (uint32_t)(uv >> 32);
    }
    uv = (uint64_t)t[8] + c;
    t[7] = (uint32_t)uv;
    t[8] = t[9] + (uint32_t)(uv >> 32);
  }
  fr o;
  LB_UNROLL for (int i = 0; i < 8; i++) o.l[i] = t[i];
  return fr_csub(o, t[8]);
}
LB_HD fr fr_sqr(const fr& a) { return fr_mul(a, a); }

LB_HD fr fr_to_mont(const fr& plain) {
  const uint32_t r2[8] = LB_FR_R2_WORDS;
  return fr_mul(plain, fr_from_words(r2));
}
LB_HD fr fr_from_mont(const fr& a) {
  fr one = fr_zero();
  one.l[0] = 1;
  return fr_mul(a, one);
}
// Montgomery form of a small integer
LB_HD fr fr_from_u32(uint32_t v) {
  fr p = fr_zero();
  p.l[0] = v;
  return fr_to_mont(p);
}

// a^e, e = 8 little-endian words (plain integer); a and the result in Montgomery form
LB_HD fr fr_pow(const fr& a, const uint32_t e[8]) {
  fr acc = fr_one();
  for (int i = 255; i >= 0; i--) {
    acc = fr_sqr(acc);
    if ((e[i >> 5] >> (i & 31)) & 1) acc = fr_mul(acc, a);
  }
  return acc;
}
// a^(r - 2): the inverse (0 -> 0).  Fermat; nothing hot inverts.
LB_HD fr fr_inv(const fr& a) {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  uint32_t e[8], bw = 0;
  LB_UNROLL for (int i = 0; i < 8; i++) e[i] = LB_SUBC(m[i], i == 0 ? 2u : 0u, bw, &bw);
  return fr_pow(a, e);
}

// 32 big-endian bytes -> Montgomery form; false if the value is >= r (out is then the value
// reduced, still a field element: callers report the element, nothing downstream misbehaves)
template <class B>
LB_HD bool fr_from_be32(fr& out, const B* b) {
  fr p;
  LB_UNROLL for (int w = 0; w < 8; w++) {
    const int o = 28 - 4 * w;
    p.l[w] = ((uint32_t)b[o] << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | (uint32_t)b[o + 3];
  }
  const bool ok = fr_lt_mod(p);
  out = fr_to_mont(p);  // fr_mul takes any 256-bit operand beside one below r
  return ok;
}
// the plain value as 8 little-endian words: the scalar layout k_g1_terms reads
LB_HD void fr_to_le_words(uint32_t out[8], const fr& a) {
  const fr p = fr_from_mont(a);
  LB_UNROLL for (int i = 0; i < 8; i++) out[i] = p.l[i];
}
// any 256-bit value (8 LE words) mod r -> Montgomery form.  2^256 < 3 r: two subtractions at most
// (hash_to_bls_field: a SHA-256 digest read as an integer)
LB_HD fr fr_reduce256(const uint32_t w[8]) {
  fr p = fr_from_words(w);
  p = fr_csub(p, 0);
  p = fr_csub(p, 0);
  return fr_to_mont(p);
}

// ------------------------------------------------------------------ radix-2 transform
// The in-order transform of lodestar_amd/kzg.py _ntt over n = 2^logn elements:
//   out[k] = sum_j a[j] w^(j k),  tw(k) = w^k for k < n / 2 (Montgomery form).
// `A` is an accessor with fr ld(uint32_t i) and void st(uint32_t i, const fr&): a flat array on
// the CPU, limb-major LDS in k_fr_intt4096.  Lane `tid` of `nthr` does its share of each phase;
// the caller puts a barrier between phases:
//   fr_ntt_bitrev;  barrier;  for s in 0 .. logn - 1: fr_ntt_stage(s);  barrier.
// The inverse transform is the same with tw(k) = w^-k and a final scaling by 1 / n.  The
// evaluations of a blob stand at the BIT-REVERSED roots, so for them fr_ntt_bitrev is skipped:
// un-reversing the input and the transform's own reversal cancel.
LB_HD uint32_t fr_bitrev(uint32_t i, int logn) {
  uint32_t r = 0;
  for (int b = 0; b < logn; b++) r |= ((i >> b) & 1u) << (logn - 1 - b);
  return r;
}
template <class A>
LB_HD void fr_ntt_bitrev(A& a, int logn, uint32_t tid, uint32_t nthr) {
  const uint32_t n = 1u << logn;
  for (uint32_t i = tid; i < n; i += nthr) {
    const uint32_t j = fr_bitrev(i, logn);
    if (i < j) {
      const fr x = a.ld(i), y = a.ld(j);
      a.st(i, y);
      a.st(j, x);
    }
  }
}
// stage s: butterflies of span m = 2^s; butterfly b pairs s0 + j and s0 + j + m with
// j = b mod m, s0 = 2 m (b div m), twiddle w^(j n / 2m)
template <class A, class T>
LB_HD void fr_ntt_stage(A& a, int logn, int s, const T& tw, uint32_t tid, uint32_t nthr) {
  const uint32_t half = 1u << (logn - 1), m = 1u << s;
  for (uint32_t b = tid; b < half; b += nthr) {
    const uint32_t j = b & (m - 1), lo = ((b >> s) << (s + 1)) + j, hi = lo + m;
    const fr u = a.ld(lo), v = fr_mul(a.ld(hi), tw(j << (logn - 1 - s)));
    a.st(lo, fr_add(u, v));
    a.st(hi, fr_sub(u, v));
  }
}
// The inverse transform's table over the blob domain's subgroup of order n = 2^logn <= 4096:
// tw[k] = w_n^-k for k < n / 2 with w_n = 7^((r - 1) / n), and tw[n / 2] = 1 / n (n / 2 + 1 entries)
#define LB_FR_INTT_TABLE_LEN(logn) ((1u << ((logn)-1)) + 1u)
LB_HD void fr_intt_table(fr* tw, int logn) {
  const uint32_t rw[8] = LB_FR_ROOT4096_WORDS;
  fr w = fr_to_mont(fr_from_words(rw));
  for (int i = logn; i < 12; i++) w = fr_sqr(w);
  const fr winv = fr_inv(w);
  const uint32_t half = 1u << (logn - 1);
  tw[0] = fr_one();
  for (uint32_t k = 1; k < half; k++) tw[k] = fr_mul(tw[k - 1], winv);
  tw[half] = fr_inv(fr_from_u32(1u << logn));
}

// ------------------------------------------------------------------ evaluate and divide
// For coefficients a[0 .. n - 1] and a point z: the suffix sums S[k] = sum_{j >= k} a[j] z^(j - k)
// (S[k] = a[k] + z S[k + 1]), which are at once the value y = p(z) = S[0] and the quotient
// (p(X) - y) / (X - z) = sum_k S[k + 1] X^k.  No division: z on the evaluation domain is no
// special case.  n / 4 lanes; lane t owns a[4 t .. 4 t + 3]:
//   fr_eq_local   T[t] = its four coefficients by Horner = S restricted to its own chunk
//   fr_eq_scan    log2(n / 4) steps d = 1, 2, 4, ...: dst[t] = src[t] + z^(4 d) src[t + d]; after
//                 the last one T[t] = S[4 t].  src and dst are distinct buffers of n / 4 values,
//                 barrier between steps, w = z^(4 d) (fr_eq_weight, squared by the caller per step)
//   fr_eq_finish  S[4 t + 3 .. 4 t] from T[t + 1], written as plain LE words: q[k - 1] = S[k]
//                 (q has n entries; q[n - 1] = 0), y = S[0]
template <class A>
LB_HD fr fr_eq_local(const A& a, const fr& z, uint32_t t) {
  fr acc = a.ld(4 * t + 3);
  LB_UNROLL for (int k = 2; k >= 0; k--) acc = fr_add(fr_mul(acc, z), a.ld(4 * t + k));
  return acc;
}
LB_HD fr fr_eq_weight(const fr& z) { return fr_sqr(fr_sqr(z)); }  // z^4: the weight of step d = 1
LB_HD fr fr_eq_scan(const fr* src, uint32_t lanes, uint32_t d, const fr& w, uint32_t t) {
  fr v = src[t];
  if (t + d < lanes) v = fr_add(v, fr_mul(w, src[t + d]));
  return v;
}
template <class A>
LB_HD void fr_eq_finish(const A& a, const fr& z, const fr* T, uint32_t lanes, uint32_t t, uint32_t* q_le,
                        uint32_t* y_le) {
  fr s = t + 1 < lanes ? T[t + 1] : fr_zero();
  LB_UNROLL for (int k = 3; k >= 0; k--) {
    s = fr_add(fr_mul(s, z), a.ld(4 * t + k));  // S[4 t + k]
    const uint32_t idx = 4 * t + k;
    if (idx > 0)
      fr_to_le_words(q_le + (size_t)8 * (idx - 1), s);
    else
      fr_to_le_words(y_le, s);
  }
  if (t + 1 == lanes) {
    LB_UNROLL for (int w = 0; w < 8; w++) q_le[(size_t)8 * (4 * lanes - 1) + w] = 0;
  }
}

// ------------------------------------------------------------------ segments: many sidecars at once
// The batched verification (lb_kzg_verify_aggregate_proof_batch) lays the polynomials of all its
// sidecars side by side; sidecar k owns polynomials off[k] .. off[k + 1] - 1.
//
// fr_seg_aggregate: element i of sum_j pw[j] poly_j over the polynomials lo <= j < hi of one
// sidecar (pw[j] = r_k^(j - lo), Montgomery form).  `poly(j, i)` and `pw(j)` are accessors; an empty
// range gives 0, the zero polynomial's element.  The caller bounds lo <= hi <= the polynomial count.
template <class P, class W>
LB_HD fr fr_seg_aggregate(const P& poly, const W& pw, uint32_t lo, uint32_t hi, uint32_t i) {
  fr acc = fr_zero();
  for (uint32_t j = lo; j < hi; j++) acc = fr_add(acc, fr_mul(pw(j), poly(j, i)));
  return acc;
}

// kzg_group_status: the status of one group of the per-blob proof form (k_kzg_check_groups,
// lb_kzg_verify_blob_proof_batch) over its blobs lo <= j < hi of n_blobs, in the order the spec's
// loop reads them: the lowest blob index with any error wins, and within a blob the commitment
// (tstatus[j]), then a blob element >= r (bstatus[j]), then the proof (tstatus[2 n_blobs + j]: the
// term that carries the proof's decode and subgroup result).  LB_OK for an empty group.
LB_HD int kzg_group_status(const int32_t* bstatus, const int32_t* tstatus, uint32_t n_blobs, uint32_t lo, uint32_t hi) {
  for (uint32_t j = lo; j < hi; j++) {
    if (tstatus[j] != LB_OK) return tstatus[j];
    if (bstatus[j] != LB_OK) return LB_BAD_SCALAR;
    if (tstatus[2 * n_blobs + j] != LB_OK) return tstatus[2 * n_blobs + j];
  }
  return LB_OK;
}

// ------------------------------------------------------------------ cells (EIP-7594, PeerDAS)
// The blob's polynomial over the 8192-point domain of w = 7^((r - 1) / 8192), in 128 cells of 64
// values: cell i holds the values at roots_brp_8192[64 i .. 64 i + 63], i.e. element t stands at
// h_i w64^brp6(t) with h_i = w^brp7(i) and w64 = w^128.  Cells 0 .. 63 are the blob itself; cells
// 64 .. 127 are p(w X) at the blob's own bit-reversed roots.
#define LB_FR_CELL 64u     // FIELD_ELEMENTS_PER_CELL
#define LB_FR_CELL_LOG 6
#define LB_FR_CELLS 128u   // CELLS_PER_EXT_BLOB
#define LB_FR_EXT 8192u    // FIELD_ELEMENTS_PER_EXT_BLOB
// the resident table of the cell calls (fr_cell_tables), in entries of one fr
#define LB_FR_CELL_TAB_FWD 0u        // w^(2 k), k < 2048: the forward 4096-point twiddles
#define LB_FR_CELL_TAB_SCALE 2048u   // w^j, j < 4096: coefficient j of p(w X)
#define LB_FR_CELL_TAB_WINV 6144u    // w^-m, m < 8192: h^-j and h^64 are entries of it
#define LB_FR_CELL_TAB_ITW 14336u    // fr_intt_table(6): the 64-point inverse transform
#define LB_FR_CELL_TAB_LEN (14336u + LB_FR_INTT_TABLE_LEN(LB_FR_CELL_LOG))

// w = 7^((r - 1) / 8192) (Montgomery form); its square is LB_FR_ROOT4096_WORDS
LB_HD fr fr_root8192() {
  const uint32_t m[8] = LB_FR_MOD_WORDS;
  uint32_t t[8], e[8];
  LB_UNROLL for (int i = 0; i < 8; i++) t[i] = m[i];
  t[0] -= 1u;  // r is odd: no borrow
  LB_UNROLL for (int i = 0; i < 8; i++) e[i] = (t[i] >> 13) | (i < 7 ? t[i + 1] << 19 : 0u);
  return fr_pow(fr_from_u32(7), e);
}
// the table above (host code: lb_kzg_load_setup, the CPU harness)
LB_HD void fr_cell_tables(fr* tab) {
  const fr w = fr_root8192(), w2 = fr_sqr(w), wi = fr_inv(w);
  tab[LB_FR_CELL_TAB_FWD] = tab[LB_FR_CELL_TAB_SCALE] = tab[LB_FR_CELL_TAB_WINV] = fr_one();
  for (uint32_t k = 1; k < 2048; k++) tab[LB_FR_CELL_TAB_FWD + k] = fr_mul(tab[LB_FR_CELL_TAB_FWD + k - 1], w2);
  for (uint32_t k = 1; k < 4096; k++) tab[LB_FR_CELL_TAB_SCALE + k] = fr_mul(tab[LB_FR_CELL_TAB_SCALE + k - 1], w);
  for (uint32_t k = 1; k < LB_FR_EXT; k++) tab[LB_FR_CELL_TAB_WINV + k] = fr_mul(tab[LB_FR_CELL_TAB_WINV + k - 1], wi);
  fr_intt_table(tab + LB_FR_CELL_TAB_ITW, LB_FR_CELL_LOG);
}
// the index into the w^-m table of h_i^64 = w^(64 brp7(i)), a 128th root of unity
LB_HD uint32_t fr_cell_h64_index(uint32_t cell_index) {
  return (LB_FR_EXT - 64u * fr_bitrev(cell_index, 7)) & (LB_FR_EXT - 1u);
}
// the plain value as 8 words whose little-endian storage is the 32 big-endian bytes
LB_HD void fr_to_be_words(uint32_t out[8], const fr& a) {
  const fr p = fr_from_mont(a);
  LB_UNROLL for (int i = 0; i < 8; i++) {
    const uint32_t v = p.l[7 - i];
    out[i] = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
  }
}

// Cells 64 .. 127 of a blob (k_fr_coset_ntt4096): from the 4096 monomial coefficients, coefficient
// j times w^j goes to slot brp12(j) (fr_coset_load: the transform's input reversal done by the
// load), twelve forward fr_ntt_stage with tw(k) = w^(2 k), and value k' of the upper half is slot
// brp12(k') (fr_coset_value: p(w X) at the blob's k'-th bit-reversed root).  Barriers between the
// phases are the caller's.
template <class A, class C, class T>
LB_HD void fr_coset_load(A& a, const C& coef, const T& scale, uint32_t tid, uint32_t nthr) {
  for (uint32_t j = tid; j < 4096u; j += nthr) a.st(fr_bitrev(j, 12), fr_mul(coef.ld(j), scale(j)));
}
template <class A>
LB_HD fr fr_coset_value(const A& a, uint32_t k) {
  return a.ld(fr_bitrev(k, 12));
}

// One cell's interpolation polynomial (k_fr_cell_interp): the 64 values stand at a bit-reversed
// coset, so six fr_ntt_stage over them as they stand with itw = fr_intt_table(6) give g(Y) = I(h Y)
// in natural order (unscaled); lane j then takes
//   weight * I_j = weight * g_j / 64 * h^-j,   h^-j = w^-(brp7(cell_index) j)   (winv: the w^-m table)
template <class T>
LB_HD fr fr_cell_descale(const fr& g, const fr& inv_n, const T& winv, uint32_t cell_index, uint32_t j, const fr& weight) {
  const uint32_t m = (fr_bitrev(cell_index, 7) * j) & (LB_FR_EXT - 1u);
  return fr_mul(fr_mul(g, inv_n), fr_mul(winv(m), weight));
}
// coefficient j of sum_k weight_k I_k over the cells lo <= k < hi of one group, always in this
// order: c(k, j) is cell k's weighted coefficient j.  An empty group gives 0.
template <class C>
LB_HD fr fr_cell_group_sum(const C& c, uint32_t lo, uint32_t hi, uint32_t j) {
  fr acc = fr_zero();
  for (uint32_t k = lo; k < hi; k++) acc = fr_add(acc, c(k, j));
  return acc;
}

// One cell's quotient (k_fr_cell_quotient): p(X) - I(X) = Q(X) (X^64 - h64) with deg I < 64, so
// q[j] = a[j + 64] + h64 q[j + 64] with q[j] = 0 for j >= n - 64: 64 independent chains, lane l
// walking j = l mod 64 from the top.  q_le: n scalars as plain LE words, the top 64 zero.
template <class A>
LB_HD void fr_cell_quotient_lane(const A& a, uint32_t n, const fr& h64, uint32_t l, uint32_t* q_le) {
  LB_UNROLL for (int w = 0; w < 8; w++) q_le[(size_t)8 * (n - 64u + l) + w] = 0;
  fr q = fr_zero();
  for (uint32_t j = n - 64u + l; j >= 64u; j -= 64u) {
    q = fr_add(a.ld(j), fr_mul(h64, q));
    fr_to_le_words(q_le + (size_t)8 * (j - 64u), q);
  }
}

// kzg_cell_group_status: the status of one verify_cell_kzg_proof_batch group in the order the spec
// reads its input: every commitment (dstatus[dlo .. dhi): the group's distinct commitments in order
// of first appearance, so the first failing position is the first failing entry), then every cell
// (cstatus[lo .. hi): an element >= r), then every proof (pstatus[lo .. hi)).  LB_OK for an empty group.
LB_HD int kzg_cell_group_status(const int32_t* dstatus, uint32_t dlo, uint32_t dhi, const int32_t* cstatus,
                                const int32_t* pstatus, uint32_t lo, uint32_t hi) {
  for (uint32_t d = dlo; d < dhi; d++)
    if (dstatus[d] != LB_OK) return dstatus[d];
  for (uint32_t j = lo; j < hi; j++)
    if (cstatus[j] != LB_OK) return LB_BAD_SCALAR;
  for (uint32_t j = lo; j < hi; j++)
    if (pstatus[j] != LB_OK) return pstatus[j];
  return LB_OK;
}

// Evaluation alone, y = p(z), where the quotient of fr_eq_* is not wanted: lane t of n / 4 takes
// its four coefficients by Horner (fr_eq_local: L[t] = sum_k a[4 t + k] z^k), then
// y = sum_t L[t] z^(4 t) folds in halves: for s = log2(n / 4) - 1 down to 0, with h = 2^s, lane
// t < h does V[t] += z^(4 h) V[t + h] (fr_ev_fold), barrier; V[0] is y.  The live lanes stay
// contiguous, so whole waves drop out step by step.  V is an accessor with ld / st over n / 4
// values; fr_ev_weight(z, s) = z^(4 * 2^s) is the weight of the step with h = 2^s.
LB_HD fr fr_ev_weight(const fr& z, int s) {
  fr w = fr_eq_weight(z);
  for (int i = 0; i < s; i++) w = fr_sqr(w);
  return w;
}
template <class V>
LB_HD void fr_ev_fold(V& v, uint32_t h, const fr& w, uint32_t t) {
  if (t < h) v.st(t, fr_add(v.ld(t), fr_mul(w, v.ld(t + h))));
}
