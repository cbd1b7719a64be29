// KZG scalar-field work on the GPU (lb_fr.h): a blob's 4096 big-endian field elements become
// Montgomery Fr in device memory, are aggregated over the blobs (sum r^j poly_j), transformed to
// monomial coefficients (inverse NTT), evaluated at a challenge and divided by (X - z), and leave
// as the plain little-endian scalars k_g1_terms reads -- so between the blob's bytes and the
// 48-byte commitment or proof nothing travels back to the host (lb_kzg_host.hip lb_kzg_blob_*,
// lb_kzg_compute_*, lb_kzg_verify_aggregate_proof).  Field elements in device buffers are 8 words
// each, array of structures.
#pragma once
#include "lb_fr.h"
#include "lb_kernels.h"
#include "lb_recover.h"

#define LB_FR_N 4096u        // FIELD_ELEMENTS_PER_BLOB
#define LB_FR_LOGN 12
#define LB_FR_WG 1024        // lanes of the one-workgroup kernels: 4 elements / 2 butterflies each
#define LB_FR_TW_LEN LB_FR_INTT_TABLE_LEN(LB_FR_LOGN)  // 2048 twiddles + 1 / 4096
#define LB_FR_INTT_LDS (LB_FR_N * 32u)                  // 131 072 B of gfx950's 163 840 per workgroup
#define LB_FR_EQ_LDS (2u * (LB_FR_N / 4) * 32u)         // two scan buffers of 1024 values

__device__ __forceinline__ fr fr_ldg(const uint32_t* __restrict__ p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  return fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void fr_stg(uint32_t* __restrict__ p, const fr& v) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
// a polynomial in global memory
struct fr_gpoly {
  const uint32_t* p;
  __device__ __forceinline__ fr ld(uint32_t i) const { return fr_ldg(p + (size_t)8 * i); }
};
struct fr_gtable {
  const uint32_t* p;
  __device__ __forceinline__ fr operator()(uint32_t k) const { return fr_ldg(p + (size_t)8 * k); }
};
// a 4096-element polynomial in LDS, limb-major: word w of element i at w * 4096 + i.  A wave's 64
// lanes touch 64 consecutive elements (or a stride-2^k comb of them in the first six stages), one
// dword each per access: consecutive banks, where 32-byte elements side by side would put every
// eighth lane on the same bank (8-way conflict).
struct fr_lds_poly {
  uint32_t* w;
  __device__ __forceinline__ fr ld(uint32_t i) const {
    fr v;
    LB_UNROLL for (int k = 0; k < 8; k++) v.l[k] = w[k * LB_FR_N + i];
    return v;
  }
  __device__ __forceinline__ void st(uint32_t i, const fr& v) {
    LB_UNROLL for (int k = 0; k < 8; k++) w[k * LB_FR_N + i] = v.l[k];
  }
};

// blobs (n_blobs x 4096 x 32 bytes, big endian) -> Montgomery Fr; status[b] = LB_BAD_SCALAR if
// blob b holds an element >= r (status zeroed by the caller; the lanes that find one all store
// the same code, so the plain stores need no ordering)
#if LB_KG(16)
__global__ void __launch_bounds__(256) k_fr_blob_load(uint32_t n_elems, const uint8_t* __restrict__ blobs,
                                                      uint32_t* __restrict__ out, int32_t* __restrict__ status) {
  const uint32_t i = lb_tid();
  if (i >= n_elems) return;
  uint8_t b[32];
  ld_bytes<32>(b, blobs + (size_t)32 * i);
  fr v;
  const bool ok = fr_from_be32(v, b);
  fr_stg(out + (size_t)8 * i, v);
  if (!ok) status[i / LB_FR_N] = LB_BAD_SCALAR;
}
#endif  // LB_KG

// agg[i] = sum_j pw[j] polys[j][i] over n_blobs polynomials of 4096 elements
#if LB_KG(16)
__global__ void __launch_bounds__(256) k_fr_aggregate(uint32_t n_blobs, const uint32_t* __restrict__ polys,
                                                      const uint32_t* __restrict__ pw, uint32_t* __restrict__ agg) {
  const uint32_t i = lb_tid();
  if (i >= LB_FR_N) return;
  fr acc = fr_zero();
  for (uint32_t j = 0; j < n_blobs; j++)
    acc = fr_add(acc, fr_mul(fr_ldg(pw + (size_t)8 * j), fr_ldg(polys + ((size_t)j * LB_FR_N + i) * 8)));
  fr_stg(agg + (size_t)8 * i, acc);
}
#endif  // LB_KG

// One workgroup per polynomial: its 4096 evaluations at the bit-reversed roots of unity -> monomial
// coefficients.  The transform's input reversal and the evaluations' own bit-reversed order cancel
// (lb_fr.h), so the twelve butterfly stages run on the values as they stand, in LDS, then every
// coefficient is scaled by 1 / 4096.  tw = fr_intt_table(12) (lb_kzg_load_setup).  out_mont /
// out_le (either may be null): Montgomery form for k_fr_eval_quotient, plain LE words for
// k_g1_terms.  LB_FR_INTT_LDS bytes of dynamic LDS.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_intt4096(const uint32_t* __restrict__ in, const uint32_t* __restrict__ tw,
                                                          uint32_t* __restrict__ out_mont, uint32_t* __restrict__ out_le) {
  extern __shared__ uint32_t lb_fr_lds[];
  const size_t base = (size_t)blockIdx.x * LB_FR_N * 8;
  fr_lds_poly A{lb_fr_lds};
  const fr_gtable T{tw};
  for (uint32_t i = threadIdx.x; i < LB_FR_N; i += LB_FR_WG) A.st(i, fr_ldg(in + base + (size_t)8 * i));
  __syncthreads();
  for (int s = 0; s < LB_FR_LOGN; s++) {
    fr_ntt_stage(A, LB_FR_LOGN, s, T, threadIdx.x, LB_FR_WG);
    __syncthreads();
  }
  const fr inv_n = T(LB_FR_N / 2);
  for (uint32_t i = threadIdx.x; i < LB_FR_N; i += LB_FR_WG) {
    const fr c = fr_mul(A.ld(i), inv_n);
    if (out_mont) fr_stg(out_mont + base + (size_t)8 * i, c);
    if (out_le) {
      uint32_t w[8];
      fr_to_le_words(w, c);
      fr_stg(out_le + base + (size_t)8 * i, fr_from_words(w));
    }
  }
}
#endif  // LB_KG

// y = p(z) and q = (p - y) / (X - z) for the 4096 coefficients `a` (Montgomery) and the point *z
// (Montgomery): lb_fr.h fr_eq_*, lane t owning a[4 t .. 4 t + 3], the ten scan steps ping-ponging
// between two LDS buffers.  q_le: 4096 scalars (plain LE words, q[4095] = 0), y_le: 8 words.
// One workgroup; LB_FR_EQ_LDS bytes of dynamic LDS.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_eval_quotient(const uint32_t* __restrict__ a, const uint32_t* __restrict__ z_mont,
                                                               uint32_t* __restrict__ q_le, uint32_t* __restrict__ y_le) {
  extern __shared__ uint32_t lb_fr_lds[];
  const uint32_t lanes = LB_FR_N / 4, t = threadIdx.x;
  fr* src = reinterpret_cast<fr*>(lb_fr_lds);
  fr* dst = src + lanes;
  const fr_gpoly A{a};
  const fr z = fr_ldg(z_mont);
  src[t] = fr_eq_local(A, z, t);
  __syncthreads();
  fr w = fr_eq_weight(z);
  for (uint32_t d = 1; d < lanes; d *= 2) {
    dst[t] = fr_eq_scan(src, lanes, d, w, t);
    __syncthreads();
    fr* x = src;
    src = dst;
    dst = x;
    w = fr_sqr(w);
  }
  fr_eq_finish(A, z, src, lanes, t, q_le, y_le);
}
#endif  // LB_KG

// ------------------------------------------------------------------ many sidecars in one pass
// lb_kzg_verify_aggregate_proof_batch: the polynomials of all sidecars stand side by side, sidecar
// k owning polynomials off[k] .. off[k + 1] - 1 (off: n_sidecars + 1 prefix sums, n_polys in all).
#define LB_FR_EV_LDS ((LB_FR_N / 4) * 32u + 16u * 32u)  // 1024 lane values + the ten step weights

struct fr_gpolys {
  const uint32_t* p;
  __device__ __forceinline__ fr operator()(uint32_t j, uint32_t i) const { return fr_ldg(p + ((size_t)j * LB_FR_N + i) * 8); }
};
// n values in LDS, limb-major like fr_lds_poly: word w of value i at w * n + i
struct fr_lds_vec {
  uint32_t* w;
  uint32_t n;
  __device__ __forceinline__ fr ld(uint32_t i) const {
    fr v;
    LB_UNROLL for (int k = 0; k < 8; k++) v.l[k] = w[k * n + i];
    return v;
  }
  __device__ __forceinline__ void st(uint32_t i, const fr& v) {
    LB_UNROLL for (int k = 0; k < 8; k++) w[k * n + i] = v.l[k];
  }
};

// agg[k][i] = sum_j pw[j] polys[j][i] over sidecar k's polynomials (pw[j] = r_k^(j - off[k])), one
// thread per element of every aggregate; a sidecar without polynomials gets the zero polynomial.
// The offsets are clamped to n_polys and to each other before anything is indexed by them.
#if LB_KG(16)
__global__ void __launch_bounds__(256) k_fr_aggregate_seg(uint32_t n_sidecars, const uint32_t* __restrict__ off, uint32_t n_polys,
                                                          const uint32_t* __restrict__ polys, const uint32_t* __restrict__ pw,
                                                          uint32_t* __restrict__ agg) {
  const uint32_t k = blockIdx.x / (LB_FR_N / 256), i = (blockIdx.x % (LB_FR_N / 256)) * 256 + threadIdx.x;
  if (k >= n_sidecars) return;
  const uint32_t hi = min(off[k + 1], n_polys), lo = min(off[k], hi);
  fr_stg(agg + ((size_t)k * LB_FR_N + i) * 8, fr_seg_aggregate(fr_gpolys{polys}, fr_gtable{pw}, lo, hi, i));
}
#endif  // LB_KG

// One workgroup per polynomial: y_k = p_k(z_k) for the 4096 coefficients coef[k] (Montgomery) and
// the point z[k] (Montgomery), each polynomial at its own point; lb_fr.h fr_eq_local and fr_ev_*.
// y_k leaves as 8 plain LE words at y_le + 8 k: a scalar of k_g1_terms.  No quotient.
// LB_FR_EV_LDS bytes of dynamic LDS.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_eval_many(const uint32_t* __restrict__ coef, const uint32_t* __restrict__ z_mont,
                                                           uint32_t* __restrict__ y_le) {
  extern __shared__ uint32_t lb_fr_lds[];
  const uint32_t lanes = LB_FR_N / 4, t = threadIdx.x, k = blockIdx.x;
  fr_lds_vec V{lb_fr_lds, lanes};
  fr_lds_vec W{lb_fr_lds + lanes * 8, 16};
  const fr_gpoly A{coef + (size_t)k * LB_FR_N * 8};
  const fr z = fr_ldg(z_mont + (size_t)8 * k);
  V.st(t, fr_eq_local(A, z, t));
  if (t < LB_FR_LOGN - 2) W.st(t, fr_ev_weight(z, (int)t));
  __syncthreads();
  for (int s = LB_FR_LOGN - 3; s >= 0; s--) {
    fr_ev_fold(V, 1u << s, W.ld((uint32_t)s), t);
    __syncthreads();
  }
  if (t == 0) {
    uint32_t w[8];
    fr_to_le_words(w, V.ld(0));
    fr_stg(y_le + (size_t)8 * k, fr_from_words(w));
  }
}
#endif  // LB_KG

// ------------------------------------------------------------------ one proof per blob
// lb_kzg_compute_blob_proofs: k_fr_eval_quotient for many polynomials, one workgroup each, polynomial
// k (coef + k * 4096 * 8, Montgomery) at its own point z_mont + 8 k.  The same suffix scan (lb_fr.h
// fr_eq_*, two LDS buffers ping-ponging, LB_FR_EQ_LDS bytes of dynamic LDS); y_k leaves as 8 plain
// LE words at y_le + 8 k and the quotient's 4096 scalars at q_le + k * 4096 * 8 (q[4095] = 0).
// No division: z on the evaluation domain is no special case.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_eval_quotient_many(const uint32_t* __restrict__ coef, const uint32_t* __restrict__ z_mont,
                                                                    uint32_t* __restrict__ q_le, uint32_t* __restrict__ y_le) {
  extern __shared__ uint32_t lb_fr_lds[];
  const uint32_t lanes = LB_FR_N / 4, t = threadIdx.x, k = blockIdx.x;
  fr* src = reinterpret_cast<fr*>(lb_fr_lds);
  fr* dst = src + lanes;
  const fr_gpoly A{coef + (size_t)k * LB_FR_N * 8};
  const fr z = fr_ldg(z_mont + (size_t)8 * k);
  src[t] = fr_eq_local(A, z, t);
  __syncthreads();
  fr w = fr_eq_weight(z);
  for (uint32_t d = 1; d < lanes; d *= 2) {
    dst[t] = fr_eq_scan(src, lanes, d, w, t);
    __syncthreads();
    fr* x = src;
    src = dst;
    dst = x;
    w = fr_sqr(w);
  }
  fr_eq_finish(A, z, src, lanes, t, q_le + (size_t)k * LB_FR_N * 8, y_le + (size_t)8 * k);
}
#endif  // LB_KG

// ------------------------------------------------------------------ cells (EIP-7594; lb_fr.h)
// lb_kzg_compute_cells, lb_kzg_compute_cell_proofs, lb_kzg_verify_cell_proof_batch.  `tab` is the
// resident table of fr_cell_tables (lb_kzg_load_setup).
#define LB_FR_CELL_BYTES (LB_FR_CELL * 32u)                 // BYTES_PER_CELL
#define LB_FR_EXT_BYTES ((size_t)LB_FR_CELLS * LB_FR_CELL_BYTES)  // one blob's 128 cells

// cells (n_cells x 64 x 32 bytes, big endian) -> Montgomery Fr; status[c] = LB_BAD_SCALAR if cell c
// holds an element >= r (status zeroed by the caller, plain stores of one code as in k_fr_blob_load)
#if LB_KG(16)
__global__ void __launch_bounds__(256) k_fr_cell_load(uint32_t n_elems, const uint8_t* __restrict__ cells,
                                                      uint32_t* __restrict__ out, int32_t* __restrict__ status) {
  const uint32_t i = lb_tid();
  if (i >= n_elems) return;
  uint8_t b[32];
  ld_bytes<32>(b, cells + (size_t)32 * i);
  fr v;
  const bool ok = fr_from_be32(v, b);
  fr_stg(out + (size_t)8 * i, v);
  if (!ok) status[i / LB_FR_CELL] = LB_BAD_SCALAR;
}
#endif  // LB_KG

// One workgroup per blob, the shape of k_fr_intt4096 (1024 lanes, LB_FR_INTT_LDS bytes of dynamic
// LDS): the blob's 4096 monomial coefficients (coef, Montgomery) -> its 128 cells.  Coefficient j
// times w^j, twelve forward stages, and the values leave as big-endian bytes in bit-reversed order
// into cells 64 .. 127 (lb_fr.h fr_coset_*); cells 0 .. 63 are the blob's own bytes, copied.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_coset_ntt4096(const uint32_t* __restrict__ coef, const uint8_t* __restrict__ blobs,
                                                               const uint32_t* __restrict__ tab, uint8_t* __restrict__ out_cells) {
  extern __shared__ uint32_t lb_fr_lds[];
  fr_lds_poly A{lb_fr_lds};
  const fr_gpoly C{coef + (size_t)blockIdx.x * LB_FR_N * 8};
  const fr_gtable SC{tab + (size_t)8 * LB_FR_CELL_TAB_SCALE}, T{tab + (size_t)8 * LB_FR_CELL_TAB_FWD};
  uint8_t* out = out_cells + (size_t)blockIdx.x * LB_FR_EXT_BYTES;
  const uint4* src = reinterpret_cast<const uint4*>(blobs + (size_t)blockIdx.x * LB_FR_N * 32);
  uint4* lower = reinterpret_cast<uint4*>(out);
  for (uint32_t i = threadIdx.x; i < LB_FR_N * 2; i += LB_FR_WG) lower[i] = src[i];
  fr_coset_load(A, C, SC, threadIdx.x, LB_FR_WG);
  __syncthreads();
  for (int s = 0; s < LB_FR_LOGN; s++) {
    fr_ntt_stage(A, LB_FR_LOGN, s, T, threadIdx.x, LB_FR_WG);
    __syncthreads();
  }
  uint32_t* upper = reinterpret_cast<uint32_t*>(out + (size_t)LB_FR_N * 32);
  for (uint32_t k = threadIdx.x; k < LB_FR_N; k += LB_FR_WG) {
    uint32_t w[8];
    fr_to_be_words(w, fr_coset_value(A, k));
    fr_stg(upper + (size_t)8 * k, fr_from_words(w));
  }
}
#endif  // LB_KG

// One wave per cell, in place over the cell's 64 Montgomery values: the 64-point inverse transform
// (six stages in LDS, one element per lane), then lane j holds weight_c I_j (fr_cell_descale;
// weight: one Montgomery value per cell, r^k of its group).  cell_index[c] < 128 (checked by the host).
#if LB_KG(16)
__global__ void __launch_bounds__(64) k_fr_cell_interp(uint32_t n_cells, uint32_t* __restrict__ cells, const uint32_t* __restrict__ cell_index,
                                                       const uint32_t* __restrict__ weight, const uint32_t* __restrict__ tab) {
  __shared__ uint32_t lds[LB_FR_CELL * 8];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  if (c >= n_cells) return;
  fr_lds_vec V{lds, LB_FR_CELL};
  const fr_gtable T{tab + (size_t)8 * LB_FR_CELL_TAB_ITW}, W{tab + (size_t)8 * LB_FR_CELL_TAB_WINV};
  uint32_t* mine = cells + ((size_t)c * LB_FR_CELL + t) * 8;
  V.st(t, fr_ldg(mine));
  __syncthreads();
  for (int s = 0; s < LB_FR_CELL_LOG; s++) {
    fr_ntt_stage(V, LB_FR_CELL_LOG, s, T, t, LB_FR_CELL);
    __syncthreads();
  }
  fr_stg(mine, fr_cell_descale(V.ld(t), T(LB_FR_CELL / 2), W, cell_index[c] & (LB_FR_CELLS - 1u), t, fr_ldg(weight + (size_t)8 * c)));
}
#endif  // LB_KG

// The per-group sum of k_fr_cell_interp's output, one thread per (group, coefficient): the cells
// off[g] .. off[g + 1] - 1 added in index order (no atomics, no floating order; lb_fr.h
// fr_cell_group_sum), NEGATED, as plain LE words at out_le + (64 g + j) * 8: the scalars of
// -RLI = -sum_j c_j [tau^j] G1 for k_g1_cell_terms.  A group may be empty (zeros) or long.
// The offsets are clamped to n_cells and to each other before anything is indexed by them.
struct fr_gcells {
  const uint32_t* p;
  __device__ __forceinline__ fr operator()(uint32_t k, uint32_t j) const { return fr_ldg(p + ((size_t)k * LB_FR_CELL + j) * 8); }
};
#if LB_KG(16)
__global__ void __launch_bounds__(64) k_fr_cell_sum(uint32_t n_groups, const uint32_t* __restrict__ off, uint32_t n_cells,
                                                    const uint32_t* __restrict__ cells, uint32_t* __restrict__ out_le) {
  const uint32_t g = blockIdx.x, j = threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t hi = min(off[g + 1], n_cells), lo = min(off[g], hi);
  uint32_t w[8];
  fr_to_le_words(w, fr_neg(fr_cell_group_sum(fr_gcells{cells}, lo, hi, j)));
  fr_stg(out_le + ((size_t)g * LB_FR_CELL + j) * 8, fr_from_words(w));
}
#endif  // LB_KG

// One wave per chosen cell of one blob: the quotient of p by X^64 - h^64 (lb_fr.h
// fr_cell_quotient_lane) from the blob's coefficients (coef, Montgomery), 4096 plain LE scalars at
// q_le + c * 4096 * 8 with the top 64 zero.  cell_index[c] < 128 (checked by the host).
#if LB_KG(16)
__global__ void __launch_bounds__(64) k_fr_cell_quotient(uint32_t n_cells, const uint32_t* __restrict__ coef, const uint32_t* __restrict__ cell_index,
                                                         const uint32_t* __restrict__ tab, uint32_t* __restrict__ q_le) {
  const uint32_t c = blockIdx.x;
  if (c >= n_cells) return;
  const fr_gtable W{tab + (size_t)8 * LB_FR_CELL_TAB_WINV};
  fr_cell_quotient_lane(fr_gpoly{coef}, LB_FR_N, W(fr_cell_h64_index(cell_index[c] & (LB_FR_CELLS - 1u))), threadIdx.x,
                        q_le + (size_t)c * LB_FR_N * 8);
}
#endif  // LB_KG

// ------------------------------------------------------------------ cell recovery (lb_recover.h)
// lb_kzg_recover_cells_and_proofs: from k_fr_cell_interp's output (unit weights) to the blob's
// coefficients.  fk: the table of fk_tables, tab: the table of fr_cell_tables; the shift s is w = tab's
// w^1, so s^k and s^-k are its w^j and w^-m entries.  mask: LB_RC_MASK_WORDS words per blob, bit i set
// where cell i is given (built by the host from the validated indices).
// 128 slots in LDS, limb-major (fr_lds_vec), with the arithmetic fk_fft_stage asks of its accessor
struct fr_lds_slots : fr_lds_vec {
  __device__ __forceinline__ fr add(const fr& u, const fr& v) const { return fr_add(u, v); }
  __device__ __forceinline__ fr sub(const fr& u, const fr& v) const { return fr_sub(u, v); }
};
// w^k v by one field product; tw: 64 Montgomery values
struct fr_gmulw {
  const uint32_t* tw;
  __device__ __forceinline__ fr operator()(const fr& v, uint32_t k) const { return fr_mul(v, fr_ldg(tw + (size_t)8 * k)); }
};

// One wave per blob: Zev[m] = Z(w128^m) and 1 / Zc[m] = 1 / Z(w w128^m), m < 128, for the vanishing
// polynomial Z of the blob's missing cells, at zev / zcinv + (128 b + m) * 8 (Montgomery).
#if LB_KG(16)
__global__ void __launch_bounds__(64) k_fr_recover_zero(uint32_t n_blobs, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ fk,
                                                        const uint32_t* __restrict__ tab, uint32_t* __restrict__ zev,
                                                        uint32_t* __restrict__ zcinv) {
  const uint32_t b = blockIdx.x;
  if (b >= n_blobs) return;
  uint32_t mk[LB_RC_MASK_WORDS];
  LB_UNROLL for (uint32_t w = 0; w < LB_RC_MASK_WORDS; w++) mk[w] = mask[b * LB_RC_MASK_WORDS + w];
  rc_zero_lane(mk, fr_gtable{fk + (size_t)8 * LB_FK_TAB_FWD_MONT}, fr_ldg(tab + (size_t)8 * (LB_FR_CELL_TAB_SCALE + 1u)), threadIdx.x,
               zev + (size_t)b * LB_FK_N * 8, zcinv + (size_t)b * LB_FK_N * 8);
}
#endif  // LB_KG

// One wave per (blob, column): blockIdx.x = 64 b + r, two points per lane as in k_fr_fk_cols.  cells:
// the call's n_cells interpolated cells (64 Montgomery values each), blob b's being off[b] ..
// off[b + 1] - 1 in ascending cell order (a position past n_cells reads cell n_cells - 1: nothing is
// indexed out of the buffer).  The column's 64 coefficients go to coef + (4096 b + 64 k + r) * 8
// (Montgomery, k_fr_fk_cols' and k_fr_ntt4096's input); a non-zero upper half stores LB_VERIFY_FAIL
// into status[b] (zeroed by the caller; plain stores of one code as in k_fr_blob_load).
#if LB_KG(16)
__global__ void __launch_bounds__(64) k_fr_recover_cols(uint32_t n_blobs, const uint32_t* __restrict__ cells, uint32_t n_cells,
                                                        const uint32_t* __restrict__ off, const uint32_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ zev, const uint32_t* __restrict__ zcinv,
                                                        const uint32_t* __restrict__ fk, const uint32_t* __restrict__ tab,
                                                        uint32_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ uint32_t lds[LB_FK_N * 8];
  const uint32_t b = blockIdx.x / LB_FK_COLS, r = blockIdx.x % LB_FK_COLS, t = threadIdx.x;
  if (b >= n_blobs || !n_cells) return;
  fr_lds_slots V{{lds, LB_FK_N}};
  const fr_gmulw FW{fk + (size_t)8 * LB_FK_TAB_FWD_MONT}, IW{fk + (size_t)8 * LB_FK_TAB_INV_MONT};
  uint32_t mk[LB_RC_MASK_WORDS];
  LB_UNROLL for (uint32_t w = 0; w < LB_RC_MASK_WORDS; w++) mk[w] = mask[b * LB_RC_MASK_WORDS + w];
  const uint32_t last = n_cells - 1u;
  const auto C = [cells, last](uint32_t k, uint32_t j) { return fr_ldg(cells + ((size_t)min(k, last) * LB_FR_CELL + j) * 8); };
  rc_col_load(V, C, mk, off[b], fr_gtable{zev + (size_t)b * LB_FK_N * 8}, r, t);
  __syncthreads();
  for (int s = 0; s < LB_FK_LOG; s++) {
    fk_fft_stage(V, s, IW, t);
    __syncthreads();
  }
  fr v[2];
  rc_take(V, fr_gtable{tab + (size_t)8 * LB_FR_CELL_TAB_SCALE}, t, v);
  __syncthreads();
  rc_put(V, t, v);
  __syncthreads();
  for (int s = 0; s < LB_FK_LOG; s++) {
    fk_fft_stage(V, s, FW, t);
    __syncthreads();
  }
  rc_take(V, fr_gtable{zcinv + (size_t)b * LB_FK_N * 8}, t, v);
  __syncthreads();
  rc_put(V, t, v);
  __syncthreads();
  for (int s = 0; s < LB_FK_LOG; s++) {
    fk_fft_stage(V, s, IW, t);
    __syncthreads();
  }
  const fr inv_n = fr_ldg(fk + (size_t)8 * LB_FK_TAB_SCALE_MONT);
  if (rc_col_store(V, fr_gtable{tab + (size_t)8 * LB_FR_CELL_TAB_WINV}, fr_sqr(inv_n), r, t, coef + (size_t)b * LB_FR_N * 8))
    status[b] = LB_VERIFY_FAIL;
}
#endif  // LB_KG

// One workgroup per blob, the shape of k_fr_intt4096 (1024 lanes, LB_FR_INTT_LDS bytes of dynamic
// LDS): the blob's 4096 monomial coefficients (coef, Montgomery) -> its 4096 big-endian elements, the
// evaluations in bit-reversed order, at out_blobs + b * 131072.  Twelve forward stages, no coset
// scale (lb_recover.h rc_blob_load); k_fr_coset_ntt4096 takes the result for the cells' first half.
#if LB_KG(16)
__global__ void __launch_bounds__(LB_FR_WG) k_fr_ntt4096(const uint32_t* __restrict__ coef, const uint32_t* __restrict__ tab,
                                                         uint8_t* __restrict__ out_blobs) {
  extern __shared__ uint32_t lb_fr_lds[];
  fr_lds_poly A{lb_fr_lds};
  const fr_gpoly C{coef + (size_t)blockIdx.x * LB_FR_N * 8};
  const fr_gtable T{tab + (size_t)8 * LB_FR_CELL_TAB_FWD};
  rc_blob_load(A, C, threadIdx.x, LB_FR_WG);
  __syncthreads();
  for (int s = 0; s < LB_FR_LOGN; s++) {
    fr_ntt_stage(A, LB_FR_LOGN, s, T, threadIdx.x, LB_FR_WG);
    __syncthreads();
  }
  uint32_t* out = reinterpret_cast<uint32_t*>(out_blobs + (size_t)blockIdx.x * LB_FR_N * 32);
  for (uint32_t k = threadIdx.x; k < LB_FR_N; k += LB_FR_WG) {
    uint32_t w[8];
    fr_to_be_words(w, fr_coset_value(A, k));
    fr_stg(out + (size_t)8 * k, fr_from_words(w));
  }
}
#endif  // LB_KG
