// The kernels of lb_kzg_compute_cells_and_proofs (lb_fk20.h: FK20 over the resident setup).
//   once per setup   k_g1_fk_gather -> k_g1_fft128 (forward)            the table X_i[r], 8192 g1j
//   per call         k_fr_fk_cols            C_i[r] / 128 as ladder scalars, 64 columns per blob
//                    k_g1_jac_terms          C_i[r] X_i[r], every ladder of the call in one launch
//                    k_g1_sum64 (lb_kzg.h)   E[r]
//                    k_g1_fft128 (inverse), k_g1_fft128 (forward, first 64 inputs)
//                    k_g1_fk_out48           affine by one inversion per wave, compressed, proof brp7(m)
// Points in device buffers are g1j SoA (soa_ld / soa_st); a point at infinity is z = 0 everywhere, in
// the table too (low-degree blobs give E[r] = O, short setups would give X = O).
#pragma once
#include "lb_fk20.h"
#include "lb_kzg_field.h"

// 128 Jacobian points in LDS, word-major like the global SoA: word w of point i at w * 128 + i
struct fk_lds_points {
  uint32_t* w;
  __device__ __forceinline__ g1j ld(uint32_t i) const {
    g1j v;
    uint32_t* o = reinterpret_cast<uint32_t*>(&v);
    LB_UNROLL for (int k = 0; k < 36; k++) o[k] = w[k * LB_FK_N + i];
    return v;
  }
  __device__ __forceinline__ void st(uint32_t i, const g1j& v) {
    const uint32_t* o = reinterpret_cast<const uint32_t*>(&v);
    LB_UNROLL for (int k = 0; k < 36; k++) w[k * LB_FK_N + i] = o[k];
  }
  __device__ __forceinline__ g1j add(const g1j& u, const g1j& v) const { return jac_add_i(u, v); }
  __device__ __forceinline__ g1j sub(const g1j& u, const g1j& v) const { return jac_add_i(u, jac_neg(v)); }
};
// w^k v by the ladder; tw: 64 scalars of 8 LE words
struct fk_g1_mulw {
  const uint32_t* tw;
  __device__ __forceinline__ g1j operator()(const g1j& v, uint32_t k) const {
    uint32_t s[8];
    LB_UNROLL for (int w = 0; w < 8; w++) s[w] = tw[8 * k + w];
    return jac_mul_u255_jac(v, s);
  }
};

// x_i[j] for the table's transforms: entry 128 i + j of `out` (8192 g1j) = setup point
// fk_setup_index(i, j) or O.  setup: the g1a SoA of lb_kzg_load_setup, setup_n >= 4096 entries.
#if LB_KG(17)
__global__ void __launch_bounds__(LB_TPB) k_g1_fk_gather(const uint32_t* __restrict__ setup, uint32_t setup_n, uint32_t* __restrict__ out) {
  const uint32_t e = lb_tid();
  if (e >= LB_FK_POINTS) return;
  const uint32_t idx = fk_setup_index(e / LB_FK_N, e % LB_FK_N);
  g1j p = jac_infinity<fp>();
  if (idx < setup_n) p = jac_from_aff(soa_ld<g1a>(setup, setup_n, idx));
  soa_st(out, LB_FK_POINTS, e, p);
}
#endif  // LB_KG

// One wave per transform t < n_tr, all seven stages (lb_fk20.h fk_fft_stage) over 128 points in LDS
// (18 KiB).  Input j < n_live is entry t in_st + j in_sj of `in` (in_cap entries), inputs from n_live
// on are O; output m goes to entry t out_st + m out_sm of `out` (out_cap entries).  tw: w^k as 64 LE
// scalars, forward or inverse (fk_tables); scale: null, or one LE scalar every output is multiplied
// by.  Nothing outside in_cap / out_cap is touched.
#if LB_KG(17)
__global__ void __launch_bounds__(64) k_g1_fft128(uint32_t n_tr, const uint32_t* __restrict__ in, uint32_t in_cap, uint32_t in_st,
                                                  uint32_t in_sj, uint32_t n_live, const uint32_t* __restrict__ tw,
                                                  const uint32_t* __restrict__ scale, uint32_t* __restrict__ out, uint32_t out_cap,
                                                  uint32_t out_st, uint32_t out_sm) {
  __shared__ uint32_t lds[36 * LB_FK_N];
  const uint32_t t = blockIdx.x, lane = threadIdx.x;
  if (t >= n_tr) return;
  fk_lds_points A{lds};
  const fk_g1_mulw M{tw};
  for (uint32_t j = lane; j < LB_FK_N; j += 64u) {
    const uint64_t idx = (uint64_t)t * in_st + (uint64_t)j * in_sj;
    A.st(fk_fft_slot(j), j < n_live && idx < in_cap ? soa_ld<g1j>(in, in_cap, (uint32_t)idx) : jac_infinity<fp>());
  }
  __syncthreads();
  for (int s = 0; s < LB_FK_LOG; s++) {
    fk_fft_stage(A, s, M, lane);
    __syncthreads();
  }
  uint32_t sc[8];
  if (scale) LB_UNROLL for (int w = 0; w < 8; w++) sc[w] = scale[w];
  for (uint32_t m = lane; m < LB_FK_N; m += 64u) {
    g1j p = A.ld(m);
    if (scale) p = jac_mul_u255_jac(p, sc);
    const uint64_t idx = (uint64_t)t * out_st + (uint64_t)m * out_sm;
    if (idx < out_cap) soa_st(out, out_cap, (uint32_t)idx, p);
  }
}
#endif  // LB_KG

// One wave per (blob, column): blockIdx.x = 64 b + i.  coef: the blobs' Montgomery coefficients
// (k_fr_intt4096), tab: fk_tables; out_le: 8192 LE scalars per blob, scalar 64 r + i = C_i[r] / 128.
#if LB_KG(17)
__global__ void __launch_bounds__(64) k_fr_fk_cols(uint32_t n_blobs, const uint32_t* __restrict__ coef, const uint32_t* __restrict__ tab,
                                                   uint32_t* __restrict__ out_le) {
  __shared__ uint32_t lds[LB_FK_N * 8];
  const uint32_t b = blockIdx.x / LB_FK_COLS, i = blockIdx.x % LB_FK_COLS, t = threadIdx.x;
  if (b >= n_blobs) return;
  fr_lds_vec V{lds, LB_FK_N};
  const fr_gtable T{tab + (size_t)8 * LB_FK_TAB_FWD_MONT};
  fk_col_load(V, fr_gpoly{coef + (size_t)b * LB_FR_N * 8}, i, t);
  __syncthreads();
  for (int s = 0; s < LB_FK_LOG; s++) {
    fr_ntt_stage(V, LB_FK_LOG, s, T, t, 64u);
    __syncthreads();
  }
  fk_col_store(V, fr_ldg(tab + (size_t)8 * LB_FK_TAB_SCALE_MONT), i, t, out_le + (size_t)b * LB_FK_POINTS * 8);
}
#endif  // LB_KG

// k_g1_terms for a Jacobian table: thread i < n takes table entry i mod table_n (g1j SoA, infinity
// allowed) times scalars[i] (8 LE words, < r) -> terms, a g1j SoA of n entries
#if LB_KG(17)
__global__ void __launch_bounds__(LB_TPB, LB_MINW) k_g1_jac_terms(uint32_t n, const uint32_t* __restrict__ table, uint32_t table_n,
                                                         const uint32_t* __restrict__ scalars, uint32_t* __restrict__ terms) {
  const uint32_t i = lb_tid();
  if (i >= n) return;
  uint32_t k[8];
  LB_UNROLL for (int w = 0; w < 8; w++) k[w] = scalars[(size_t)8 * i + w];
  soa_st(terms, n, i, jac_mul_u255_jac(soa_ld<g1j>(table, table_n, i % table_n), k));
}
#endif  // LB_KG

// The proofs leave: point t of `in` (g1j SoA of n entries, n a multiple of 128: transform t div 128,
// output m = t mod 128) -> affine with ONE inversion per wave (fp_inv_block), compressed to
// out48 + 48 (128 (t div 128) + brp7(m)): the proof of cell brp7(m).  One wave per block.
#if LB_KG(17)
__global__ void __launch_bounds__(64) k_g1_fk_out48(uint32_t n, const uint32_t* __restrict__ in, uint8_t* __restrict__ out48) {
  const uint32_t t = lb_tid();
  const bool live = t < n;
  const g1j p = live ? soa_ld<g1j>(in, n, t) : jac_infinity<fp>();
  const bool inf = jac_is_inf(p);
  const fp zi = fp_inv_block(inf ? fp_one() : p.z), zi2 = fp_sqr(zi);
  if (!live) return;
  const g1a a{fp_mul(p.x, zi2), fp_mul(fp_mul(p.y, zi2), zi)};
  uint8_t b[48];
  g1_compress48(b, a, inf);
  uint8_t* o = out48 + (size_t)48 * ((t & ~(LB_FK_N - 1u)) + fr_bitrev(t & (LB_FK_N - 1u), LB_FK_LOG));
  for (int k = 0; k < 48; k++) o[k] = b[k];
}
#endif  // LB_KG
