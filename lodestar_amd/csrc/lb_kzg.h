// KZG commitments over BLS12-381 (the c-kzg calls behind packages/beacon-node/src/util/kzg.ts:15-65:
// blobToKzgCommitment, computeAggregateKzgProof, verifyAggregateKzgProof).
// The GPU does the group work: G1 linear combinations of the resident trusted setup (a 4 096-term
// multi-scalar multiplication per commitment or proof) or of given points (the aggregated
// commitment), and the proof check as one two-pair pairing product.  The scalar-field work
// (inverse FFT, aggregation, evaluations, quotients) is either the caller's (lodestar_amd/kzg.py
// and js/kzg.js with field = "host", over lb_g1_lincomb / lb_kzg_verify_proof) or the GPU's too:
// the k_fr_* kernels of lb_kzg_field.h behind the blob-level calls (lb_kzg_blob_to_commitment,
// lb_kzg_compute_aggregate_proof, lb_kzg_verify_aggregate_proof ...), which feed the kernels below
// from device memory.  The Fiat-Shamir transcript is hashed on the host either way.
//
// Setup layout: the monomial-form points [tau^i] G1 (what Lodestar's trusted_setup.bin holds; a
// commitment to p(X) = sum a_i X^i is sum a_i [tau^i] G1, the same point as the spec's Lagrange
// form sum p(w_i) L_i(tau) G1) as a g1a SoA table; [tau^0] G2 and [tau^1] G2 as two g2a, and where
// the setup file has it [tau^64] G2 as a third (the cell proofs of EIP-7594 pair against it).
#pragma once
#include "lb_fr.h"  // kzg_group_status
#include "lb_kernels.h"

// one point per thread: P_i (table entry i, or 48 compressed bytes) times scalar i (32 bytes,
// little endian, < r) -> Jacobian SoA terms.  Given points are curve- and subgroup-checked
// (lb_curve.h g1_in_subgroup_r).
#if LB_KG(7)
__global__ void __launch_bounds__(LB_TPB, LB_MINW) k_g1_terms(uint32_t n, const uint8_t* __restrict__ pts48,
                                                     const uint32_t* __restrict__ table, uint32_t table_cap,
                                                     const uint32_t* __restrict__ scalars,
                                                     uint32_t* __restrict__ terms, int32_t* __restrict__ status) {
  const uint32_t i = lb_tid();
  if (i >= n) return;
  g1a p;
  bool inf = false;
  int st = LB_OK;
  if (pts48) {
    uint8_t b[48];
    ld_bytes<48>(b, pts48 + (size_t)48 * i);
    st = g1_decompress48(b, p, inf);
    if (st == LB_OK && !inf && !g1_in_subgroup_r(p)) st = LB_POINT_NOT_IN_GROUP;
  } else {
    p = soa_ld<g1a>(table, table_cap, i);
  }
  uint32_t k[8];
  LB_UNROLL for (int w = 0; w < 8; w++) k[w] = scalars[(size_t)8 * i + w];
  g1j t = jac_infinity<fp>();
  if (st == LB_OK && !inf) t = jac_mul_u256(p, k);
  soa_st(terms, n, i, t);
  status[i] = st;
}
#endif  // LB_KG

// out[b] = sum of in[64 b .. 64 b + 63] (SoA, strides n_in / n_out), one wave per block.  (The tree
// is wave_sum64's, kept in its own words: through the helper this kernel's registers come out in
// another order.)
#if LB_KG(7)
__global__ void __launch_bounds__(64) k_g1_sum64(uint32_t n_in, const uint32_t* __restrict__ in, uint32_t n_out,
                                                 uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  g1j v = i < n_in ? soa_ld<g1j>(in, n_in, i) : jac_infinity<fp>();
  for (int l = 5; l >= 0; l--) {
    const unsigned d = 1u << l;
    const g1j o{fp_shfl_down(v.x, d), fp_shfl_down(v.y, d), fp_shfl_down(v.z, d)};
    if (threadIdx.x < d) v = jac_add_i(v, o);
  }
  if (threadIdx.x == 0) soa_st(out, n_out, blockIdx.x, v);
}
#endif  // LB_KG

// element 0 of a g1j SoA (stride n) -> 48 compressed bytes
#if LB_KG(7)
__global__ void __launch_bounds__(64) k_g1_out48(const uint32_t* __restrict__ in, uint32_t n, uint8_t* __restrict__ out48) {
  if (threadIdx.x != 0) return;
  const g1j v = soa_ld<g1j>(in, n, 0);
  g1a a;
  const bool fin = jac_to_aff(a, v);
  uint8_t b[48];
  g1_compress48(b, a, !fin);
  for (int k = 0; k < 48; k++) out48[k] = b[k];
}
#endif  // LB_KG

// decode the trusted setup into the resident tables (G1 points: curve + subgroup checks)
#if LB_KG(7)
__global__ void __launch_bounds__(LB_TPB, LB_MINW) k_kzg_setup_g1(uint32_t n, const uint8_t* __restrict__ in48,
                                                         uint32_t* __restrict__ table, uint32_t cap,
                                                         int32_t* __restrict__ status) {
  const uint32_t i = lb_tid();
  if (i >= n) return;
  uint8_t b[48];
  ld_bytes<48>(b, in48 + (size_t)48 * i);
  g1a a;
  bool inf;
  int st = g1_decompress48(b, a, inf);
  if (st == LB_OK && inf) st = LB_PK_IS_INFINITY;
  if (st == LB_OK && !g1_in_subgroup_r(a)) st = LB_POINT_NOT_IN_GROUP;
  if (st != LB_OK) {
    a.x = fp_zero();
    a.y = fp_zero();
  }
  soa_st(table, cap, i, a);
  status[i] = st;
}
#endif  // LB_KG
#if LB_KG(7)
__global__ void __launch_bounds__(64) k_kzg_setup_g2(uint32_t n, const uint8_t* __restrict__ in96, uint32_t* __restrict__ g2,
                                                     int32_t* __restrict__ status) {
  const uint32_t i = threadIdx.x;
  if (i >= n || i >= 3) return;  // [tau^0] G2, [tau^1] G2 and, for the cell calls, [tau^64] G2
  uint8_t b[96];
  ld_bytes<96>(b, in96 + (size_t)96 * i);
  g2a a;
  bool inf;
  int st = g2_decompress96(b, a, inf);
  if (st == LB_OK && (inf || !g2_in_subgroup(jac_from_aff(a)))) st = LB_POINT_NOT_IN_GROUP;
  uint32_t* w = reinterpret_cast<uint32_t*>(&a);
  for (int k = 0; k < 48; k++) g2[48 * i + k] = w[k];
  status[i] = st;
}
#endif  // LB_KG

// The two-pair pairing check that every KZG verification ends in,
//   e(Q, -[tau^0] G2) e(P, G) == 1,   G = setup G2 point gi (g2: [tau^0] G2, [tau^1] G2, [tau^64] G2 as g2a),
// for one wave (the block) on the wave engine; every lane calls it, with what LANE 0 computed: the
// status st, and Q and P in affine form with their finite flags (the other lanes' arguments are not
// read).  Lane 0's values go to all lanes through LDS, since the Miller-or-one choices must be
// wave-uniform; a point at infinity pairs to 1, so Q = P = O accepts and exactly one of them at
// infinity rejects.  Returns what the kernel writes: 1 / 0, or -st for a bad status, which never
// reaches the pairing (Q and P need not be set then).  Uses areas LBW_A(0) and LBW_A(7).
__device__ __forceinline__ int w_kzg_pairing_check(fp* S, int st, const g1a& qa, bool qfin, const g1a& pa, bool pfin,
                                                   const uint32_t* __restrict__ g2, int gi) {
  __shared__ int st_sh, qinf_sh, pinf_sh;
  const int lane = threadIdx.x;
  const g2a* G = reinterpret_cast<const g2a*>(g2);
  if (lane == 0) {
    st_sh = st;
    qinf_sh = qfin ? 0 : 1;
    pinf_sh = pfin ? 0 : 1;
    if (st == LB_OK) w_stage_pair(S, qa, g2a_neg(G[0]));  // -G2
  }
  __syncthreads();
  const int st_u = st_sh, qinf = qinf_sh, pinf = pinf_sh;
  __syncthreads();
  if (st_u != LB_OK) return -st_u;
  if (qinf)
    w_set_one(S, LBW_A(0));
  else
    w_miller(S, LBW_A(0));
  if (lane == 0) w_stage_pair(S, pa, G[gi]);
  __syncthreads();
  if (pinf)
    w_set_one(S, LBW_A(7));
  else
    w_miller(S, LBW_A(7));
  w_mul(S, LBW_A(0), LBW_A(0), LBW_A(7));
  w_final_exp(S, LBW_A(0), LBW_A(0));
  return w_is_one(S, LBW_A(0)) ? 1 : 0;
}

// verify_kzg_proof_impl: e(C - [y] G1, -G2) e(pi, [tau] G2 - [z] G2) == 1, rewritten with the
// scalar moved to G1 (bilinearity): e(Q, -G2) e(pi, [tau] G2) == 1 with Q = C - [y] G1 + [z] pi.
// Lanes 0 and 1 compute [y] G1 and [z] pi side by side, lanes 2 and 3 the subgroup checks of C
// and pi (c-kzg rejects commitments and proofs outside G1); the two Miller loops and the final
// exponentiation run on the wave engine.  io[0..47] C, [48..95] pi, scalars y, z (8 LE words
// each); g2 = [tau^0] G2, [tau^1] G2 (g2a).  *ok = 1 / 0, or -code for a bad point encoding.
#if LB_KG(5)
__global__ void __launch_bounds__(64) k_kzg_check(const uint8_t* __restrict__ io, const uint32_t* __restrict__ yz,
                                                  const uint32_t* __restrict__ g2, int32_t* __restrict__ ok) {
  LBW_SHARED_ML(S);
  __shared__ g1j sh[2];
  __shared__ int grp_sh[2];
  const int lane = threadIdx.x;
  w_init_consts(S, LBW_PROGS_ALL);
  g1a c, pi;
  bool cinf = false, pinf = false;
  int st = LB_OK;
  {
    uint8_t b[48];
    for (int k = 0; k < 48; k++) b[k] = io[k];
    st = g1_decompress48(b, c, cinf);
    if (st == LB_OK) {
      for (int k = 0; k < 48; k++) b[k] = io[48 + k];
      st = g1_decompress48(b, pi, pinf);
    }
  }
  if (lane < 2) {
    uint32_t k[8];
    for (int w = 0; w < 8; w++) k[w] = yz[8 * lane + w];
    const g1a base = lane == 0 ? g1a{fp_load(LB_G1X), fp_load(LB_G1Y)} : pi;
    const bool binf = lane == 1 && pinf;
    sh[lane] = (st == LB_OK && !binf) ? jac_mul_u256(base, k) : jac_infinity<fp>();
  } else if (lane < 4) {
    const bool isc = lane == 2;
    const bool skip = st != LB_OK || (isc ? cinf : pinf);
    grp_sh[lane - 2] = skip || g1_in_subgroup_r(isc ? c : pi) ? 1 : 0;
  }
  __syncthreads();
  if (st == LB_OK && !(grp_sh[0] && grp_sh[1])) st = LB_POINT_NOT_IN_GROUP;
  g1a qa;
  bool qfin = false;
  if (lane == 0) {
    g1j q = cinf ? jac_infinity<fp>() : jac_from_aff(c);
    q = jac_add_i(q, jac_neg(sh[0]));
    q = jac_add_i(q, sh[1]);
    qfin = jac_to_aff(qa, q);
  }
  const int verdict = w_kzg_pairing_check(S, st, qa, qfin, pi, !pinf, g2, 1);
  if (lane == 0) *ok = verdict;
}
#endif  // LB_KG

// The same check for many sidecars at once (lb_kzg_verify_aggregate_proof_batch): one wave per
// sidecar k, which owns blobs off[k] .. off[k + 1] - 1 of n_blobs.  The scalar multiplications and
// the subgroup checks ran before, in one k_g1_terms launch over n_blobs + 2 n points:
//   [0, n_blobs)            the commitments C_j, scalars r_k^j
//   n_blobs + k             the proof pi_k, scalar x_k
//   n_blobs + n + k         the G1 generator, scalar y_k
// (pts48, terms as a g1j SoA of that many entries, tstatus).  Here: the sidecar's status by the single
// call's precedence (a blob element >= r, bstatus; the first failing commitment; the proof), then
// T_k = sum_j [r_k^j] C_j - [y_k] G1 + [x_k] pi_k and e(T_k, -G2) e(pi_k, [tau] G2) == 1 on the
// wave engine.  ok[k] = 1 / 0, or -code; a sidecar with a bad status never reaches the pairing.
// The offsets are clamped to n_blobs and to each other before anything is indexed by them.
#if LB_KG(5)
__global__ void __launch_bounds__(64) k_kzg_check_many(uint32_t n, const uint32_t* __restrict__ off, uint32_t n_blobs,
                                                       const int32_t* __restrict__ bstatus, const uint8_t* __restrict__ pts48,
                                                       const uint32_t* __restrict__ terms, const int32_t* __restrict__ tstatus,
                                                       const uint32_t* __restrict__ g2, int32_t* __restrict__ ok) {
  LBW_SHARED_ML(S);
  const int lane = threadIdx.x;
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  w_init_consts(S, LBW_PROGS_ALL);
  const uint32_t n_pts = n_blobs + 2 * n, i_pi = n_blobs + k, i_g = n_blobs + n + k;
  const uint32_t hi = min(off[k + 1], n_blobs), lo = min(off[k], hi);
  // the sidecar's terms: its commitments, then [x] pi, then [y] G1 (subtracted); 64 at a time
  const uint32_t m = hi - lo + 2;
  g1j v = jac_infinity<fp>();
  for (uint32_t q = lane; q < m; q += 64) {
    const uint32_t idx = q + 2 < m ? lo + q : (q + 2 == m ? i_pi : i_g);
    g1j t = soa_ld<g1j>(terms, n_pts, idx);
    if (q + 1 == m) t = jac_neg(t);
    v = jac_add_i(v, t);
  }
  v = wave_sum64(v, threadIdx.x);
  int st = LB_OK;
  g1a qa, pi;
  bool qfin = false, pinf = false;
  if (lane == 0) {
    for (uint32_t j = lo; j < hi && st == LB_OK; j++)
      if (bstatus[j] != LB_OK) st = LB_BAD_SCALAR;
    for (uint32_t j = lo; j < hi && st == LB_OK; j++) st = tstatus[j];
    if (st == LB_OK) st = tstatus[i_pi];
    if (st == LB_OK) {
      // pi in affine form for its Miller loop (its status is LB_OK: it decodes)
      uint8_t b[48];
      ld_bytes<48>(b, pts48 + (size_t)48 * i_pi);
      st = g1_decompress48(b, pi, pinf);
      qfin = jac_to_aff(qa, v);
    }
  }
  const int verdict = w_kzg_pairing_check(S, st, qa, qfin, pi, !pinf, g2, 1);
  if (lane == 0) ok[k] = verdict;
}
#endif  // LB_KG

// The per-blob proof form (Deneb's verify_blob_kzg_proof_batch; lb_kzg_verify_blob_proof_batch): one
// wave per group k, which owns blobs off[k] .. off[k + 1] - 1 of n_blobs, each with its own
// commitment C_j and proof pi_j.  With r the group's combiner and i = j - off[k], the ladders ran
// before, in one k_g1_terms launch over 3 n_blobs + n points:
//   [0, n_blobs)              C_j,   scalar r^i
//   n_blobs + j               pi_j,  scalar r^i z_j
//   2 n_blobs + j             pi_j,  scalar r^i
//   3 n_blobs + k             the G1 generator, scalar sum_i r^i y_j
// (terms as a g1j SoA of that many entries, tstatus).  Here: the group's status (lb_fr.h
// kzg_group_status: lowest blob first; commitment, blob element, proof), then
//   T = sum [r^i] C_j + sum [r^i z_j] pi_j - [sum r^i y_j] G1,   P = sum [r^i] pi_j
// and e(T, -G2) e(P, [tau] G2) == 1 on the wave engine; either point may be infinity (constant blobs
// with infinity proofs make T infinity), an empty group accepts.  ok[k] = 1 / 0, or -code; a group
// with a bad status never reaches the pairing.  The offsets are clamped to n_blobs and to each
// other before anything is indexed by them.
#if LB_KG(5)
__global__ void __launch_bounds__(64) k_kzg_check_groups(uint32_t n, const uint32_t* __restrict__ off, uint32_t n_blobs,
                                                         const int32_t* __restrict__ bstatus, const uint32_t* __restrict__ terms,
                                                         const int32_t* __restrict__ tstatus, const uint32_t* __restrict__ g2,
                                                         int32_t* __restrict__ ok) {
  LBW_SHARED_ML(S);
  const int lane = threadIdx.x;
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  w_init_consts(S, LBW_PROGS_ALL);
  const uint32_t n_pts = 3 * n_blobs + n, i_g = 3 * n_blobs + k;
  const uint32_t hi = min(off[k + 1], n_blobs), lo = min(off[k], hi);
  const uint32_t m = hi - lo;
  // T: the group's C terms, its z pi terms, then the generator term (subtracted); 64 at a time
  g1j v = jac_infinity<fp>();
  for (uint32_t q = lane; q < 2 * m + 1; q += 64) {
    const uint32_t idx = q < m ? lo + q : (q < 2 * m ? n_blobs + lo + (q - m) : i_g);
    g1j t = soa_ld<g1j>(terms, n_pts, idx);
    if (q == 2 * m) t = jac_neg(t);
    v = jac_add_i(v, t);
  }
  v = wave_sum64(v, threadIdx.x);
  // P: the group's pi terms
  g1j u = jac_infinity<fp>();
  for (uint32_t q = lane; q < m; q += 64) u = jac_add_i(u, soa_ld<g1j>(terms, n_pts, 2 * n_blobs + lo + q));
  u = wave_sum64(u, threadIdx.x);
  int st = LB_OK;
  g1a qa, pa;
  bool qfin = false, pfin = false;
  if (lane == 0) {
    st = kzg_group_status(bstatus, tstatus, n_blobs, lo, hi);
    if (st == LB_OK) {
      qfin = jac_to_aff(qa, v);
      pfin = jac_to_aff(pa, u);
    }
  }
  const int verdict = w_kzg_pairing_check(S, st, qa, qfin, pa, pfin, g2, 1);
  if (lane == 0) ok[k] = verdict;
}
#endif  // LB_KG

// ------------------------------------------------------------------ cell proofs (EIP-7594)
// k_g1_terms for the cell batch, both kinds of point in ONE launch (two launches of these
// latency-bound ladders would run one after the other): thread i < n_pts takes given point i (48
// compressed bytes, curve- and subgroup-checked) times scalars[i]; thread n_pts + t takes table entry
// t mod period times tscalars[t] (lb_kzg_verify_cell_proof_batch: period 64, group g's negated
// interpolation coefficients at 64 g .. 64 g + 63 against [tau^0 .. tau^63] G1).  Scalars: 8 LE words,
// < r.  terms: a g1j SoA of n_pts + n_tab entries, status alike (LB_OK for setup points, which were
// checked on load).  period <= table_cap (checked by the host).
#if LB_KG(7)
__global__ void __launch_bounds__(LB_TPB, LB_MINW) k_g1_cell_terms(uint32_t n_pts, const uint8_t* __restrict__ pts48,
                                                          const uint32_t* __restrict__ scalars, uint32_t n_tab,
                                                          const uint32_t* __restrict__ table, uint32_t table_cap, uint32_t period,
                                                          const uint32_t* __restrict__ tscalars, uint32_t* __restrict__ terms,
                                                          int32_t* __restrict__ status) {
  const uint32_t i = lb_tid(), n = n_pts + n_tab;
  if (i >= n) return;
  g1a p;
  bool inf = false;
  int st = LB_OK;
  const uint32_t* sc;
  if (i < n_pts) {
    uint8_t b[48];
    ld_bytes<48>(b, pts48 + (size_t)48 * i);
    st = g1_decompress48(b, p, inf);
    if (st == LB_OK && !inf && !g1_in_subgroup_r(p)) st = LB_POINT_NOT_IN_GROUP;
    sc = scalars + (size_t)8 * i;
  } else {
    p = soa_ld<g1a>(table, table_cap, (i - n_pts) % period);
    sc = tscalars + (size_t)8 * (i - n_pts);
  }
  uint32_t k[8];
  LB_UNROLL for (int w = 0; w < 8; w++) k[w] = sc[w];
  g1j t = jac_infinity<fp>();
  if (st == LB_OK && !inf) t = jac_mul_u256(p, k);
  soa_st(terms, n, i, t);
  status[i] = st;
}
#endif  // LB_KG

// verify_cell_kzg_proof_batch (lb_kzg_verify_cell_proof_batch): one wave per group k, which owns cells
// off[k] .. off[k + 1] - 1 of n_cells and the distinct commitments doff[k] .. doff[k + 1] - 1 of
// n_comms.  With r the group's combiner, i the cell's place in its group and h its coset shift, the
// ladders ran before, in one k_g1_cell_terms launch over 2 n_cells + n_comms given points and 64 n
// table entries (terms as a g1j SoA of that many entries, tstatus):
//   [0, n_cells)                  pi_j,  scalar r^i
//   n_cells + j                   pi_j,  scalar r^i h^64
//   2 n_cells + d                 distinct commitment d, scalar the sum of its cells' r^i
//   2 n_cells + n_comms + 64 k + t   [tau^t] G1, scalar the NEGATED summed interpolation coefficient t
// Here: the group's status
// (lb_fr.h kzg_cell_group_status: commitments, cells, proofs), then
//   LL = sum [r^i] pi_j,   RL = sum of the commitment terms + sum [r^i h^64] pi_j + the 64 table terms
// and e(RL, -G2) e(LL, [tau^64] G2) == 1 on the wave engine; either point may be infinity, an empty
// group accepts.  g2 = [tau^0] G2, [tau^1] G2, [tau^64] G2.  ok[k] = 1 / 0, or -code; a group with a bad
// status never reaches the pairing.  All offsets are clamped before anything is indexed by them.
#if LB_KG(5)
__global__ void __launch_bounds__(64) k_kzg_check_cells(uint32_t n, const uint32_t* __restrict__ off, uint32_t n_cells,
                                                        const uint32_t* __restrict__ doff, uint32_t n_comms,
                                                        const int32_t* __restrict__ cstatus, const uint32_t* __restrict__ terms,
                                                        const int32_t* __restrict__ tstatus, const uint32_t* __restrict__ g2,
                                                        int32_t* __restrict__ ok) {
  LBW_SHARED_ML(S);
  const int lane = threadIdx.x;
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  w_init_consts(S, LBW_PROGS_ALL);
  const uint32_t n_given = 2 * n_cells + n_comms, n_pts = n_given + 64 * n;
  const uint32_t hi = min(off[k + 1], n_cells), lo = min(off[k], hi), m = hi - lo;
  const uint32_t dhi = min(doff[k + 1], n_comms), dlo = min(doff[k], dhi), d = dhi - dlo;
  // RL: the commitment terms, the h^64 pi terms, the 64 table terms; 64 at a time
  g1j v = jac_infinity<fp>();
  for (uint32_t q = lane; q < d + m + 64; q += 64) {
    const uint32_t idx = q < d ? 2 * n_cells + dlo + q : (q < d + m ? n_cells + lo + (q - d) : n_given + 64 * k + (q - d - m));
    v = jac_add_i(v, soa_ld<g1j>(terms, n_pts, idx));
  }
  v = wave_sum64(v, threadIdx.x);
  // LL: the pi terms
  g1j u = jac_infinity<fp>();
  for (uint32_t q = lane; q < m; q += 64) u = jac_add_i(u, soa_ld<g1j>(terms, n_pts, lo + q));
  u = wave_sum64(u, threadIdx.x);
  int st = LB_OK;
  g1a qa, pa;
  bool qfin = false, pfin = false;
  if (lane == 0) {
    st = kzg_cell_group_status(tstatus + 2 * n_cells, dlo, dhi, cstatus, tstatus, lo, hi);
    if (st == LB_OK) {
      qfin = jac_to_aff(qa, v);
      pfin = jac_to_aff(pa, u);
    }
  }
  const int verdict = w_kzg_pairing_check(S, st, qa, qfin, pa, pfin, g2, 2);
  if (lane == 0) ok[k] = verdict;
}
#endif  // LB_KG
