// BLS12-381 field tower for gfx950: Fp (12 x u32 Montgomery limbs), Fp2 = Fp[u]/(u^2+1),
// Fp6 = Fp2[v]/(v^3 - (1+u)), Fp12 = Fp6[w]/(w^2 - v).
//
// Replaces the blst field layer that @chainsafe/blst@0.2.7 runs under
// packages/beacon-node/src/chain/bls/maybeBatch.ts:18-37.
// Every element is kept fully reduced in [0, p) in Montgomery form (R = 2^384), so
// equality is limb equality and serialisation is one Montgomery multiply away.
// The 32x32->64 multiply-accumulate chains lower to v_mad_u64_u32 on gfx950.
#pragma once
#include "lb_common.h"
#include "lb_consts.h"

struct fp {
  uint32_t v[12];
};
struct fp2 {
  fp c0, c1;
};
struct fp6 {
  fp2 c0, c1, c2;
};
struct fp12 {
  fp6 c0, c1;
};

// ------------------------------------------------------------------ Fp basics
LB_HD fp fp_load(const uint32_t* c) {
  fp r;
  LB_UNROLL for (int i = 0; i < 12; i++) r.v[i] = c[i];
  return r;
}
LB_HD fp2 fp2_load(const uint32_t* c) {
  fp2 r;
  r.c0 = fp_load(c);
  r.c1 = fp_load(c + 12);
  return r;
}
LB_HD fp fp_zero() {
  fp r;
  LB_UNROLL for (int i = 0; i < 12; i++) r.v[i] = 0;
  return r;
}
LB_HD fp fp_one() { return fp_load(LB_ONE); }

LB_HD bool fp_is_zero(const fp& a) {
  uint32_t t = 0;
  LB_UNROLL for (int i = 0; i < 12; i++) t |= a.v[i];
  return t == 0;
}
LB_HD bool fp_eq(const fp& a, const fp& b) {
  uint32_t t = 0;
  LB_UNROLL for (int i = 0; i < 12; i++) t |= a.v[i] ^ b.v[i];
  return t == 0;
}
LB_HD fp fp_select(bool c, const fp& a, const fp& b) {
  fp r;
  LB_UNROLL for (int i = 0; i < 12; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// r = a - p if a >= p (a given as 12 limbs + carry word)
LB_HD fp fp_reduce_once(const uint32_t* t, uint32_t top) {
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  uint32_t s[12];
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) s[j] = LB_SUBC(t[j], Pl[j], br, &br);
  bool ge = (top != 0) || (br == 0);
  fp r;
  LB_UNROLL for (int j = 0; j < 12; j++) r.v[j] = ge ? s[j] : t[j];
  return r;
}

LB_HD fp fp_add(const fp& a, const fp& b) {
  uint32_t t[12];
  uint32_t c = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) t[j] = LB_ADDC(a.v[j], b.v[j], c, &c);
  return fp_reduce_once(t, c);
}

LB_HD fp fp_sub(const fp& a, const fp& b) {
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  uint32_t t[12];
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) t[j] = LB_SUBC(a.v[j], b.v[j], br, &br);
  // if borrow, add p back
  uint32_t m = 0u - br;
  fp r;
  uint32_t c = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) r.v[j] = LB_ADDC(t[j], Pl[j] & m, c, &c);
  return r;
}

LB_HD fp fp_neg(const fp& a) { return fp_sub(fp_zero(), a); }
LB_HD fp fp_dbl(const fp& a) { return fp_add(a, a); }

// Montgomery multiplication a*b/R mod p, 12 x 32-bit limbs, operand scanning in carry-save
// form.  Textbook CIOS threads one carry through all 288 multiply-adds, so a lone wave waits
// on a 288-deep v_mad_u64_u32 dependency chain.  Here every row keeps the carry out of limb j
// *pending* for limb j+1 of the next row: u = a_i*b_j + t_j + cc_j <= (2^32-1)^2 + 2(2^32-1)
// < 2^64, so each row's 12 products are independent and the chain is ~7 deep per row.
// After the multiply row nothing is pending into limb 0, so m = t_0 * (-p^-1) mod 2^32 is
// exact; the reduction row zeroes limb 0 and the state shifts down one limb.
LB_HD fp fp_mul_body(const fp& a, const fp& b) {
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  uint32_t t[13], cc[14];
  LB_UNROLL for (int j = 0; j < 13; j++) t[j] = 0;
  LB_UNROLL for (int j = 0; j < 14; j++) cc[j] = 0;
  LB_UNROLL for (int i = 0; i < 12; i++) {
    uint32_t n[14];
    n[0] = 0;
    LB_UNROLL for (int j = 0; j < 12; j++) {
      uint64_t u = (uint64_t)a.v[i] * b.v[j] + t[j] + cc[j];
      t[j] = (uint32_t)u;
      n[j + 1] = (uint32_t)(u >> 32);
    }
    {
      uint64_t u = (uint64_t)t[12] + cc[12];
      t[12] = (uint32_t)u;
      n[13] = (uint32_t)(u >> 32) + cc[13];
    }
    // reduction row: limb 0 has no pending carry now
    uint32_t m = t[0] * LB_PINV;
    uint32_t r[14];
    r[0] = 0;
    LB_UNROLL for (int j = 0; j < 12; j++) {
      uint64_t u = (uint64_t)m * Pl[j] + t[j] + n[j];
      t[j] = (uint32_t)u;
      r[j + 1] = (uint32_t)(u >> 32);
    }
    {
      uint64_t u = (uint64_t)t[12] + n[12];
      t[12] = (uint32_t)u;
      r[13] = (uint32_t)(u >> 32) + n[13];
    }
    // divide by 2^32: limb 0 is zero; pending carries shift with the limbs
    LB_UNROLL for (int j = 0; j < 12; j++) t[j] = t[j + 1];
    t[12] = 0;
    LB_UNROLL for (int j = 0; j < 13; j++) cc[j] = r[j + 1];
    cc[13] = 0;
  }
  // resolve the pending carries (value < 2p < 2^382, so nothing escapes limb 12)
  uint32_t o[12];
  uint32_t c = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) o[j] = LB_ADDC(t[j], cc[j], c, &c);
  uint32_t top = t[12] + cc[12] + c;
  return fp_reduce_once(o, top);
}

// Montgomery multiplication on 14 x 28-bit unsaturated limbs (same R = 2^384 contract as
// fp_mul_body).  With 28-bit limbs every partial product is < 2^56 and a column collects at most
// 28 of them plus a 2^36 carry, so a 64-bit column accumulator never overflows: each of the 392
// products is ONE carry-free v_mad_u64_u32 (acc = a*b + acc), against 288 MADs + 288 carry adds
// for 32-bit limbs, and the rows carry nothing but one shift per row.
// R stays 2^384 although 14 rows divide by 2^392: the second operand is unpacked as b * 2^8
// (b * 2^8 < 2^392 fits), so the result is a b 2^8 / 2^392 = a b / R.  For a b < R p the output is
// below 2p (as for fp_mul_body), and one conditional subtraction finishes it.
LB_HD uint32_t lb_bits28(const uint32_t* w, int off) {  // bits [off, off + 28) of a 12-word value
  const int q = off >> 5, r = off & 31;
  const uint32_t lo = q < 12 ? w[q] : 0u;
  const uint32_t hi = q + 1 < 12 ? w[q + 1] : 0u;
  return (r ? ((lo >> r) | (hi << (32 - r))) : lo) & 0x0fffffffu;
}
LB_HD fp fp_mul28(const fp& a, const fp& b) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  uint32_t A[14], B[14];
  LB_UNROLL for (int k = 0; k < 14; k++) A[k] = lb_bits28(a.v, 28 * k);
  B[0] = (b.v[0] << 8) & 0x0fffffffu;
  LB_UNROLL for (int k = 1; k < 14; k++) B[k] = lb_bits28(b.v, 28 * k - 8);
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    LB_UNROLL for (int j = 0; j < 14; j++) acc[i + j] += (uint64_t)A[i] * B[j];
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) acc[i + j] += (uint64_t)m * P28[j];
    acc[i + 1] += acc[i] >> 28;  // column i is now a multiple of 2^28
  }
  uint32_t r[14];
  LB_UNROLL for (int k = 0; k < 13; k++) {
    r[k] = (uint32_t)acc[14 + k] & 0x0fffffffu;
    acc[15 + k] += acc[14 + k] >> 28;
  }
  r[13] = (uint32_t)acc[27];  // < 2^18: the value is below 2p < 2^382
  uint32_t o[12];
  LB_UNROLL for (int w = 0; w < 12; w++) {
    const int l = (32 * w) / 28, s = 32 * w - 28 * l;  // s <= 24: two limbs cover a word
    o[w] = (r[l] >> s) | (r[l + 1] << (28 - s));
  }
  return fp_reduce_once(o, 0u);
}

// Montgomery squaring on the same 14 x 28-bit limbs: 105 products instead of 196 for a * a.
// The operand is unpacked once as a' = a * 2^4, so a'^2 = a^2 2^8 and the 2^392 reduction again
// yields a^2 / R.  Off-diagonal products use 2 a'_i (29 bits): a column holds at most 7 of them
// (< 2^57 each), one square, 14 reduction products (< 2^56) and a 2^36 carry: < 2^61.
LB_HD fp fp_sqr28(const fp& a) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  uint32_t A[14], D[14];
  A[0] = (a.v[0] << 4) & 0x0fffffffu;
  LB_UNROLL for (int k = 1; k < 14; k++) A[k] = lb_bits28(a.v, 28 * k - 4);
  LB_UNROLL for (int k = 0; k < 14; k++) D[k] = A[k] << 1;
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    acc[2 * i] += (uint64_t)A[i] * A[i];
    LB_UNROLL for (int j = i + 1; j < 14; j++) acc[i + j] += (uint64_t)D[i] * A[j];
  }
  LB_UNROLL for (int i = 0; i < 14; i++) {
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) acc[i + j] += (uint64_t)m * P28[j];
    acc[i + 1] += acc[i] >> 28;
  }
  uint32_t r[14];
  LB_UNROLL for (int k = 0; k < 13; k++) {
    r[k] = (uint32_t)acc[14 + k] & 0x0fffffffu;
    acc[15 + k] += acc[14 + k] >> 28;
  }
  r[13] = (uint32_t)acc[27];
  uint32_t o[12];
  LB_UNROLL for (int w = 0; w < 12; w++) {
    const int l = (32 * w) / 28, s = 32 * w - 28 * l;
    o[w] = (r[l] >> s) | (r[l + 1] << (28 - s));
  }
  return fp_reduce_once(o, 0u);
}

#if defined(__HIPCC__)
// Out of line on the GPU: one body shared by every call site keeps the pipeline kernels inside
// the instruction cache and compile time bounded.  Operands and result travel as 16-wide
// vectors, which the AMDGPU calling convention keeps in VGPRs (a 48-byte struct would be
// passed through scratch memory).
typedef uint32_t lb_v16u __attribute__((ext_vector_type(16)));
__device__ __forceinline__ lb_v16u fp_pack(const fp& a) {
  lb_v16u r;
  LB_UNROLL for (int i = 0; i < 12; i++) r[i] = a.v[i];
  r[12] = r[13] = r[14] = r[15] = 0;
  return r;
}
__device__ __forceinline__ fp fp_unpack(lb_v16u a) {
  fp r;
  LB_UNROLL for (int i = 0; i < 12; i++) r.v[i] = a[i];
  return r;
}
static __device__ __attribute__((noinline)) lb_v16u fp_mul_v(lb_v16u a, lb_v16u b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_pack(fp_mul28(fp_unpack(a), fp_unpack(b)));
#else
  return fp_pack(fp_mul_body(fp_unpack(a), fp_unpack(b)));
#endif
}
__host__ __device__ __forceinline__ fp fp_mul(const fp& a, const fp& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_unpack(fp_mul_v(fp_pack(a), fp_pack(b)));
#else
  return fp_mul_body(a, b);
#endif
}
static __device__ __attribute__((noinline)) lb_v16u fp_sqr_v(lb_v16u a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_pack(fp_sqr28(fp_unpack(a)));
#else
  return fp_pack(fp_mul_body(fp_unpack(a), fp_unpack(a)));
#endif
}
__host__ __device__ __forceinline__ fp fp_sqr(const fp& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_unpack(fp_sqr_v(fp_pack(a)));
#else
  return fp_mul_body(a, a);
#endif
}
#else
static inline fp fp_mul(const fp& a, const fp& b) {
  LB_COUNT_MUL();
  return fp_mul28(a, b);
}
// counted as one Fp multiplication (the roofline's unit stays the 300-MAC product)
static inline fp fp_sqr(const fp& a) {
  LB_COUNT_MUL();
  return fp_sqr28(a);
}
#endif

// small-constant multiples via additions
LB_HD fp fp_mul3(const fp& a) { return fp_add(fp_dbl(a), a); }
LB_HD fp fp_mul4(const fp& a) { return fp_dbl(fp_dbl(a)); }
LB_HD fp fp_mul8(const fp& a) { return fp_dbl(fp_mul4(a)); }

LB_HD fp fp_to_mont(const fp& a) { return fp_mul(a, fp_load(LB_R2)); }
LB_HD fp fp_from_mont(const fp& a) {
  fp one = fp_zero();
  one.v[0] = 1;
  return fp_mul(a, one);
}

// a^e for a constant exponent held in (constant) memory, bit top_bit set, by a sliding window
// of 4 bits over the odd powers a, a^3, ..., a^15: for the 379-bit sqrt exponents 378
// squarings + 86 multiplications instead of 378 + 228.  Exponent bits, window values and table
// indices are wave-uniform (scalar control flow on the GPU); the table is read through a switch
// so it stays in registers.
LB_HD fp lb_tab8(const fp* t, uint32_t k) {
  switch (k) {
    case 0: return t[0];
    case 1: return t[1];
    case 2: return t[2];
    case 3: return t[3];
    case 4: return t[4];
    case 5: return t[5];
    case 6: return t[6];
    default: return t[7];
  }
}
// Inline products for the exponentiation chains (fenced so the compiler keeps one product's
// columns live at a time): a lone lane's out-of-line product costs ~1.42 us of latency against
// ~1.05 us inline, and ~7 % more issue (tools/ubench/fpmul_ps.hip, profiles/r3_variants_ab.txt).
LB_HD fp fp_mul_inl(const fp& a, const fp& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
  const fp r = fp_mul28(a, b);
  __builtin_amdgcn_sched_barrier(0);
  return r;
#else
  return fp_mul(a, b);
#endif
}
LB_HD fp fp_sqr_inl(const fp& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
  const fp r = fp_sqr28(a);
  __builtin_amdgcn_sched_barrier(0);
  return r;
#else
  return fp_sqr(a);
#endif
}
// Limb-resident exponentiation chains.  fp_mul28 / fp_sqr28 spend ~110 of their 632 / 506 VALU
// instructions unpacking 12 x 32-bit operands into 28-bit limbs, repacking the result and
// reducing it below p.  A chain of products can stay in limbs: with Montgomery radix R' = 2^392
// (the 14 rows' own radix) the limbs of a * 2^8 ARE the R'-form of a's value (x R 2^8 = x R'),
// and a product's 14 output limbs feed the next product directly.  Values are not reduced between
// products: for inputs below 2^390 the output (ab + mp) / R' is below 2^388 + p, so every limb stays
// below 2^28 and the column bounds of fp_mul28 / fp_sqr28 hold.  The end converts back with one
// product by R mod p (r R / R' = r / 2^8 = x^e R), repacks and reduces once.
// Host test builds (-DLB_FP28_CHECK, tests/native/fp2_28_check.cpp) verify the two bounds this form
// rests on.  (1) On the actual values: no 64-bit column overflows (checked against a 128-bit sum)
// and a product's top limb stays below 2^28.  (2) For the Fp2 layer below, on the worst case: every
// fp28 carries an upper bound per limb (ub) and on its value in units of p (vb); the operations
// propagate them and assert the column, borrow and value conditions on the bounds themselves, so a
// run of straight-line formulas proves them for every input, not for the inputs of the run.
#if defined(LB_FP28_CHECK)
#include <stdio.h>
#include <stdlib.h>
#define LB_CHK(...) __VA_ARGS__
#define LB_CHK_ASSERT(c)                                                                \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "fp28 bound violated: %s (%s:%d)\n", #c, __FILE__, __LINE__);     \
      abort();                                                                          \
    }                                                                                   \
  } while (0)
// acc + x * y stays below 2^64
#define LB_COL_CHK(acc, x, y) \
  LB_CHK_ASSERT((unsigned __int128)(acc) + (unsigned __int128)(x) * (y) <= (unsigned __int128)~0ull)
#else
#define LB_CHK(...)
#define LB_CHK_ASSERT(c) ((void)0)
#define LB_COL_CHK(acc, x, y) ((void)0)
#endif
struct fp28 {
  uint32_t l[14];
  LB_CHK(uint64_t ub[14]; double vb;)
};
LB_HD fp28 fp28_mul_raw(const fp28& a, const fp28& b) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], a.l[i], b.l[j]);
      acc[i + j] += (uint64_t)a.l[i] * b.l[j];
    }
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], m, P28[j]);
      acc[i + j] += (uint64_t)m * P28[j];
    }
    LB_COL_CHK(acc[i + 1], acc[i] >> 28, 1u);
    acc[i + 1] += acc[i] >> 28;
  }
  fp28 r;
  LB_UNROLL for (int k = 0; k < 13; k++) {
    r.l[k] = (uint32_t)acc[14 + k] & 0x0fffffffu;
    LB_COL_CHK(acc[15 + k], acc[14 + k] >> 28, 1u);
    acc[15 + k] += acc[14 + k] >> 28;
  }
  LB_CHK_ASSERT(acc[27] < (1ull << 28));  // the value is below 2^392
  r.l[13] = (uint32_t)acc[27];
  return r;
}
LB_HD fp28 fp28_sqr_raw(const fp28& a) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  uint32_t D[14];
  LB_UNROLL for (int k = 0; k < 14; k++) D[k] = a.l[k] << 1;
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    LB_CHK_ASSERT(a.l[i] < (1u << 31));  // D[i] = 2 a_i fits a word
    LB_COL_CHK(acc[2 * i], a.l[i], a.l[i]);
    acc[2 * i] += (uint64_t)a.l[i] * a.l[i];
    LB_UNROLL for (int j = i + 1; j < 14; j++) {
      LB_COL_CHK(acc[i + j], D[i], a.l[j]);
      acc[i + j] += (uint64_t)D[i] * a.l[j];
    }
  }
  LB_UNROLL for (int i = 0; i < 14; i++) {
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], m, P28[j]);
      acc[i + j] += (uint64_t)m * P28[j];
    }
    LB_COL_CHK(acc[i + 1], acc[i] >> 28, 1u);
    acc[i + 1] += acc[i] >> 28;
  }
  fp28 r;
  LB_UNROLL for (int k = 0; k < 13; k++) {
    r.l[k] = (uint32_t)acc[14 + k] & 0x0fffffffu;
    LB_COL_CHK(acc[15 + k], acc[14 + k] >> 28, 1u);
    acc[15 + k] += acc[14 + k] >> 28;
  }
  LB_CHK_ASSERT(acc[27] < (1ull << 28));  // the value is below 2^392
  r.l[13] = (uint32_t)acc[27];
  return r;
}
LB_HD fp28 fp28_mul(const fp28& a, const fp28& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
  const fp28 r = fp28_mul_raw(a, b);
  __builtin_amdgcn_sched_barrier(0);
  return r;
#else
  return fp28_mul_raw(a, b);
#endif
}
LB_HD fp28 fp28_sqr(const fp28& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
  const fp28 r = fp28_sqr_raw(a);
  __builtin_amdgcn_sched_barrier(0);
  return r;
#else
  return fp28_sqr_raw(a);
#endif
}
LB_HD fp28 lb_tab8_28(const fp28* t, uint32_t k) {
  switch (k) {
    case 0: return t[0];
    case 1: return t[1];
    case 2: return t[2];
    case 3: return t[3];
    case 4: return t[4];
    case 5: return t[5];
    case 6: return t[6];
    default: return t[7];
  }
}
// Sliding window of 4 bits: the 8 odd powers on the stack (448 B per lane, ~170 VGPRs: three waves
// per SIMD in the signature decode).  A 3-bit window keeps its 4 powers in registers, no stack, but
// needs 222 VGPRs (two waves) and ~10 % more decode instructions: 1.5 % lower throughput at 7 in
// flight (profiles/r4_regress_ab.txt), for 268 -> 53 MB of decode traffic per batch.
LB_HD fp fp_pow_const_28(const fp& a, const uint32_t* e, int top_bit) {
  constexpr int WIN = 4;
  fp28 tab[8];
  tab[0].l[0] = (a.v[0] << 8) & 0x0fffffffu;  // the limbs of a * 2^8: a's value in R'-form
  LB_UNROLL for (int k = 1; k < 14; k++) tab[0].l[k] = lb_bits28(a.v, 28 * k - 8);
  const fp28 a2 = fp28_sqr(tab[0]);
  // the odd powers through a loop the unroller leaves rolled (its body is too large for the
  // unroller's budget): the table indexed dynamically, on the stack (cache-resident)
  for (int k = 1; k < 8; k++) tab[k] = fp28_mul(tab[k - 1], a2);
  auto bit = [&](int i) -> uint32_t { return (e[i >> 5] >> (i & 31)) & 1u; };
  fp28 r = tab[0];
  bool first = true;
  int i = top_bit;
  while (i >= 0) {
    if (!bit(i)) {
      if (!first) r = fp28_sqr(r);
      i--;
      continue;
    }
    int j = i - (WIN - 1) > 0 ? i - (WIN - 1) : 0;
    while (!bit(j)) j++;
    uint32_t val = 0;
    for (int k = i; k >= j; k--) val = (val << 1) | bit(k);
    if (first) {
      r = lb_tab8_28(tab, val >> 1);
      first = false;
    } else {
      for (int k = i; k >= j; k--) r = fp28_sqr(r);
      r = fp28_mul(r, lb_tab8_28(tab, val >> 1));
    }
    i = j - 1;
  }
  // back to R-form: r * (R mod p) / R' = r / 2^8, below 2p; repack and reduce once
  const fp one = fp_one();
  fp28 c;
  LB_UNROLL for (int k = 0; k < 14; k++) c.l[k] = lb_bits28(one.v, 28 * k);
  const fp28 t = fp28_mul(r, c);
  uint32_t o[12];
  LB_UNROLL for (int w = 0; w < 12; w++) {
    const int l = (32 * w) / 28, s = 32 * w - 28 * l;
    o[w] = (t.l[l] >> s) | (t.l[l + 1] << (28 - s));
  }
  return fp_reduce_once(o, 0u);
}

// ---- Fp2 over fp28: curve formulas that stay in 28-bit limbs from product to product.
// A value is any non-negative integer congruent to x R' (R' = 2^392), never reduced below p, in
// limbs that may exceed 28 bits between products.  Two bounds keep this sound; with
// R' / p = 2520.2 and p / 2^364 = 106513.1 both are stated in small numbers:
//   value   a product's output is (S + m p) / R' with m < R', S the sum of its operand products:
//           out < S / R' + p, that is out / p < 1 + (S / p^2) / 2520.  Operands of a few tens of p
//           give outputs of 1..3 p, and S < 2520^2 p^2 keeps every output below 2^392.
//   column  a 64-bit column collects 14 limb products per Fp product, 14 reduction terms below
//           2^56 and one carry below 2^37: for limb bounds La, Lb (one product) or La Lb + Lc Ld
//           summed (two products)   14 (La Lb + Lc Ld) + 14 (2^28 - 1)^2 + 2^37 <= 2^64 - 1,
//           e.g. both sides of both products up to 2^29.5, or 2^31 against 2^28.
// Linear operations work limb by limb, without carry chain, compare or select:
//   a - b = a + K - b,  K = C p in a borrowed form: limb 0 + 2^S, limbs 1..12 + 2^S - 2^(S-28),
//   limb 13 - 2^(S-28) (the same integer), so limbs 0..12 of K are at least 2^S - 2^(S-28) and
//   cover any b whose limbs are below that; limb 13 of K must cover b's top limb, which bounds C
//   from below by b's value.  The result grows by C p in value and 2^S + 2^28 per limb.
//   fp28_norm is the one carry pass that brings limbs 0..12 back below 2^28 (the value stays).
// The bounds are derived per call site (lb_curve.h: g2_dbl_lean28, g2_madd_lean28) and enforced by
// the LB_FP28_CHECK host build on the worst case, see above.
LB_HD constexpr uint32_t lb_k28_limb(uint32_t c, int s, int i) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  uint64_t carry = 0, k = 0;
  for (int j = 0; j <= i; j++) {
    const uint64_t t = (uint64_t)c * P28[j] + carry;
    k = j < 13 ? (t & 0x0fffffffu) : t;
    carry = t >> 28;
  }
  const uint64_t b = 1ull << s, bh = 1ull << (s - 28);
  return (uint32_t)(i == 0 ? k + b : i < 13 ? k + b - bh : k - bh);
}
#define LB_K28(C, S)                                                                                          \
  {lb_k28_limb(C, S, 0), lb_k28_limb(C, S, 1), lb_k28_limb(C, S, 2),  lb_k28_limb(C, S, 3),  lb_k28_limb(C, S, 4), \
   lb_k28_limb(C, S, 5), lb_k28_limb(C, S, 6), lb_k28_limb(C, S, 7),  lb_k28_limb(C, S, 8),  lb_k28_limb(C, S, 9), \
   lb_k28_limb(C, S, 10), lb_k28_limb(C, S, 11), lb_k28_limb(C, S, 12), lb_k28_limb(C, S, 13)}

#if defined(LB_FP28_CHECK)
// top-limb bound of a value below vb p whose limbs 0..12 are non-negative
static inline uint64_t fp28_chk_top(double vb) { return (uint64_t)(vb * 106513.2) + 1; }
// a value known to be below vb p with limbs 0..12 below 2^28
static inline void fp28_chk_set(fp28& a, double vb) {
  for (int k = 0; k < 13; k++) a.ub[k] = 0x0fffffffu;
  a.ub[13] = fp28_chk_top(vb) < 0x0fffffffu ? fp28_chk_top(vb) : 0x0fffffffu;
  a.vb = vb;
}
static inline void fp28_chk_in(const fp28& a) {
  for (int k = 0; k < 14; k++) LB_CHK_ASSERT(a.l[k] <= a.ub[k]);
}
// worst-case columns of (a b + c d) / R' (c, d may be null) and the bounds of the result
static inline void fp28_chk_mac(const fp28& a, const fp28& b, const fp28* c, const fp28* d, fp28& r) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  typedef unsigned __int128 u128;
  const u128 lim = (u128)~0ull;
  fp28_chk_in(a), fp28_chk_in(b);
  if (c) fp28_chk_in(*c), fp28_chk_in(*d);
  u128 col[29];
  for (int k = 0; k < 29; k++) col[k] = 0;
  for (int i = 0; i < 14; i++) {
    for (int j = 0; j < 14; j++) {
      col[i + j] += (u128)a.ub[i] * b.ub[j] + (u128)0x0fffffffu * P28[j];
      if (c) col[i + j] += (u128)c->ub[i] * d->ub[j];
    }
    LB_CHK_ASSERT(col[i] <= lim);
    col[i + 1] += col[i] >> 28;
  }
  for (int k = 14; k < 28; k++) {
    LB_CHK_ASSERT(col[k] <= lim);
    col[k + 1] += col[k] >> 28;
  }
  const double s = a.vb * b.vb + (c ? c->vb * d->vb : 0.0);
  const double vb = (1.0 + s / 2520.0) * (1.0 + 1e-9);
  LB_CHK_ASSERT(vb < 2520.0);  // below 2^392
  fp28_chk_set(r, vb);
}
#endif

struct fp2_28 {
  fp28 c0, c1;
};
LB_HD fp28 fp28_add(const fp28& a, const fp28& b) {
  fp28 r;
  LB_UNROLL for (int k = 0; k < 14; k++) {
    r.l[k] = a.l[k] + b.l[k];
    LB_CHK(r.ub[k] = a.ub[k] + b.ub[k]; LB_CHK_ASSERT(r.ub[k] <= 0xffffffffull);)
  }
  LB_CHK(r.vb = a.vb + b.vb;)
  return r;
}
template <int N>  // N a: 2, 3, 4, 8 by shifts and adds
LB_HD fp28 fp28_muls(const fp28& a) {
  fp28 r;
  LB_UNROLL for (int k = 0; k < 14; k++) {
    r.l[k] = N == 3 ? (a.l[k] << 1) + a.l[k] : a.l[k] << (N == 2 ? 1 : N == 4 ? 2 : 3);
    LB_CHK(r.ub[k] = N * a.ub[k]; LB_CHK_ASSERT(r.ub[k] <= 0xffffffffull);)
  }
  LB_CHK(r.vb = N * a.vb;)
  return r;
}
// a + K - b, K = C p borrowed at 2^S: needs b's limbs 0..12 <= 2^S - 2^(S-28) and b's top limb <=
// K's; the value grows by at most C p.  fp28_kminus is K - b alone.
template <uint32_t C, int S>
LB_HD fp28 fp28_kminus(const fp28& b) {
  constexpr uint32_t K[14] = LB_K28(C, S);
  fp28 r;
  LB_CHK(if (b.ub[13] > K[13]) fprintf(stderr, "K = %u p does not cover a value of %.2f p\n", C, b.vb);)
  LB_UNROLL for (int k = 0; k < 14; k++) {
    r.l[k] = K[k] - b.l[k];
    LB_CHK(LB_CHK_ASSERT(b.ub[k] <= K[k]); r.ub[k] = K[k];)
  }
  LB_CHK(r.vb = C;)
  return r;
}
template <uint32_t C, int S>
LB_HD fp28 fp28_sub(const fp28& a, const fp28& b) {
  constexpr uint32_t K[14] = LB_K28(C, S);
  fp28 r;
  LB_CHK(if (b.ub[13] > K[13]) fprintf(stderr, "K = %u p does not cover a value of %.2f p\n", C, b.vb);)
  LB_UNROLL for (int k = 0; k < 14; k++) {
    r.l[k] = a.l[k] + K[k] - b.l[k];
    LB_CHK(LB_CHK_ASSERT(b.ub[k] <= K[k]); r.ub[k] = a.ub[k] + K[k]; LB_CHK_ASSERT(r.ub[k] <= 0xffffffffull);)
  }
  LB_CHK(r.vb = a.vb + C;)
  return r;
}
// one carry pass: limbs 0..12 below 2^28 again, the top limb takes the rest
LB_HD fp28 fp28_norm(const fp28& a) {
  fp28 r;
  uint32_t c = 0;
  LB_CHK(uint64_t cb = 0;)
  LB_UNROLL for (int k = 0; k < 13; k++) {
    const uint32_t t = a.l[k] + c;
    LB_CHK(LB_CHK_ASSERT(a.ub[k] + cb <= 0xffffffffull); cb = (a.ub[k] + cb) >> 28;)
    r.l[k] = t & 0x0fffffffu;
    c = t >> 28;
  }
  r.l[13] = a.l[13] + c;
  LB_CHK(const uint64_t top = a.ub[13] + cb; fp28_chk_set(r, a.vb); if (top < r.ub[13]) r.ub[13] = top;)
  return r;
}
// a b / R' and (a b + c d) / R': one set of 28 columns, one reduction; fenced like fp28_mul
LB_HD fp28 fp28_mulx(const fp28& a, const fp28& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
#endif
  fp28 r = fp28_mul_raw(a, b);
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
#endif
  LB_CHK(fp28_chk_mac(a, b, nullptr, nullptr, r);)
  return r;
}
LB_HD fp28 fp28_mac2(const fp28& a, const fp28& b, const fp28& c, const fp28& d) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
#endif
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], a.l[i], b.l[j]);
      acc[i + j] += (uint64_t)a.l[i] * b.l[j];
    }
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], c.l[i], d.l[j]);
      acc[i + j] += (uint64_t)c.l[i] * d.l[j];
    }
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) {
      LB_COL_CHK(acc[i + j], m, P28[j]);
      acc[i + j] += (uint64_t)m * P28[j];
    }
    LB_COL_CHK(acc[i + 1], acc[i] >> 28, 1u);
    acc[i + 1] += acc[i] >> 28;
  }
  fp28 r;
  LB_UNROLL for (int k = 0; k < 13; k++) {
    r.l[k] = (uint32_t)acc[14 + k] & 0x0fffffffu;
    LB_COL_CHK(acc[15 + k], acc[14 + k] >> 28, 1u);
    acc[15 + k] += acc[14 + k] >> 28;
  }
  LB_CHK_ASSERT(acc[27] < (1ull << 28));
  r.l[13] = (uint32_t)acc[27];
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
#endif
  LB_CHK(fp28_chk_mac(a, b, &c, &d, r);)
  return r;
}

// conversions.  fp28_from_fp: the 12-word Montgomery value a = x R as plain limbs (below p) times
// 2^400 mod p: x R 2^400 / R' = x R', below 1.0004 p.  fp28_from_fp_shift: the limbs of a 2^8, no
// product, but a value up to 256 p: for operands that meet a small partner in a product at once.
// fp28_to_fp: one product by R mod p (r R / R' = x R, below 2 p for r below 2520 p), repacked and
// reduced once: the canonical 12 words.
LB_HD fp28 fp28_one() {
  const uint32_t c[14] = {LB_R28_ONE_0, LB_R28_ONE_1, LB_R28_ONE_2, LB_R28_ONE_3, LB_R28_ONE_4,  LB_R28_ONE_5,  LB_R28_ONE_6,
                          LB_R28_ONE_7, LB_R28_ONE_8, LB_R28_ONE_9, LB_R28_ONE_10, LB_R28_ONE_11, LB_R28_ONE_12, LB_R28_ONE_13};
  fp28 r;
  LB_UNROLL for (int k = 0; k < 14; k++) r.l[k] = c[k];
  LB_CHK(fp28_chk_set(r, 1.0);)
  return r;
}
LB_HD fp28 fp28_zero() {
  fp28 r;
  LB_UNROLL for (int k = 0; k < 14; k++) r.l[k] = 0;
  LB_CHK(fp28_chk_set(r, 1.0);)
  return r;
}
LB_HD fp28 fp28_from_fp_shift(const fp& a) {
  fp28 r;
  r.l[0] = (a.v[0] << 8) & 0x0fffffffu;
  LB_UNROLL for (int k = 1; k < 14; k++) r.l[k] = lb_bits28(a.v, 28 * k - 8);
  LB_CHK(fp28_chk_set(r, 256.0);)
  return r;
}
LB_HD fp28 fp28_from_fp(const fp& a) {
  const uint32_t c[14] = {LB_R28_IN_0, LB_R28_IN_1, LB_R28_IN_2, LB_R28_IN_3, LB_R28_IN_4,  LB_R28_IN_5,  LB_R28_IN_6,
                          LB_R28_IN_7, LB_R28_IN_8, LB_R28_IN_9, LB_R28_IN_10, LB_R28_IN_11, LB_R28_IN_12, LB_R28_IN_13};
  fp28 x, k;
  LB_UNROLL for (int i = 0; i < 14; i++) x.l[i] = lb_bits28(a.v, 28 * i), k.l[i] = c[i];
  LB_CHK(fp28_chk_set(x, 1.0); fp28_chk_set(k, 1.0);)
  return fp28_mulx(x, k);
}
LB_HD fp fp28_to_fp(const fp28& a) {
  const fp one = fp_one();
  fp28 c;
  LB_UNROLL for (int k = 0; k < 14; k++) c.l[k] = lb_bits28(one.v, 28 * k);
  LB_CHK(fp28_chk_set(c, 1.0);)
  const fp28 t = fp28_mulx(a, c);
  LB_CHK_ASSERT(t.vb < 2.0);
  uint32_t o[12];
  LB_UNROLL for (int w = 0; w < 12; w++) {
    const int l = (32 * w) / 28, s = 32 * w - 28 * l;
    o[w] = (t.l[l] >> s) | (t.l[l + 1] << (28 - s));
  }
  return fp_reduce_once(o, 0u);
}
// a == 0 (mod p) on the redundant form, by converting down: the Montgomery reduction alone,
// t = (a + m p) / R' < a / R' + p, is congruent to a / R' and below 2 p for every a below 2^392,
// so t is 0 or p exactly when p divides a; t's limbs are canonical (13 masked, the rest on top).
LB_HD bool fp28_is_zero(const fp28& a) {
  const uint32_t P28[14] = {LB_P28_0, LB_P28_1, LB_P28_2, LB_P28_3, LB_P28_4,  LB_P28_5,  LB_P28_6,
                            LB_P28_7, LB_P28_8, LB_P28_9, LB_P28_10, LB_P28_11, LB_P28_12, LB_P28_13};
  LB_CHK(fp28_chk_in(a); LB_CHK_ASSERT(a.vb < 2520.0);)
  uint64_t acc[28];
  LB_UNROLL for (int k = 0; k < 28; k++) acc[k] = k < 14 ? a.l[k] : 0;
  LB_UNROLL for (int i = 0; i < 14; i++) {
    const uint32_t m = ((uint32_t)acc[i] * LB_PINV28) & 0x0fffffffu;
    LB_UNROLL for (int j = 0; j < 14; j++) acc[i + j] += (uint64_t)m * P28[j];  // < 2^32 + 14 2^56 + 2^37
    acc[i + 1] += acc[i] >> 28;
  }
  uint32_t z = 0, e = 0;
  LB_UNROLL for (int k = 0; k < 14; k++) {
    const uint32_t t = k < 13 ? ((uint32_t)acc[14 + k] & 0x0fffffffu) : (uint32_t)acc[27];
    if (k < 13) acc[15 + k] += acc[14 + k] >> 28;
    z |= t;
    e |= t ^ P28[k];
  }
  return z == 0 || e == 0;
}

// Fp2 = Fp[u] / (u^2 + 1) on the form above.  C, S of a product describe its SECOND operand (the
// K that covers b.c1, or a.c1 for the square): choose it as the operand with the smaller bounds.
LB_HD fp2_28 fp2_28_add(const fp2_28& a, const fp2_28& b) { return fp2_28{fp28_add(a.c0, b.c0), fp28_add(a.c1, b.c1)}; }
template <int N>
LB_HD fp2_28 fp2_28_muls(const fp2_28& a) {
  return fp2_28{fp28_muls<N>(a.c0), fp28_muls<N>(a.c1)};
}
template <uint32_t C, int S>
LB_HD fp2_28 fp2_28_sub(const fp2_28& a, const fp2_28& b) {
  return fp2_28{fp28_sub<C, S>(a.c0, b.c0), fp28_sub<C, S>(a.c1, b.c1)};
}
LB_HD fp2_28 fp2_28_norm(const fp2_28& a) { return fp2_28{fp28_norm(a.c0), fp28_norm(a.c1)}; }
// (a0 + a1 u)(b0 + b1 u) without Karatsuba: c0 = a0 b0 + a1 (K - b1), c1 = a0 b1 + a1 b0, each
// accumulated into one set of columns and reduced once (4 x 196 + 2 x 196 multiply-adds; no
// additions or subtractions around the products but the 14 that form K - b1)
template <uint32_t C, int S>
LB_HD fp2_28 fp2_28_mul(const fp2_28& a, const fp2_28& b) {
  const fp28 nb1 = fp28_kminus<C, S>(b.c1);
  fp2_28 r;
  r.c0 = fp28_mac2(a.c0, b.c0, a.c1, nb1);
  r.c1 = fp28_mac2(a.c0, b.c1, a.c1, b.c0);
  return r;
}
// c0 = (a0 + a1)(a0 + K - a1), c1 = (2 a0) a1
template <uint32_t C, int S>
LB_HD fp2_28 fp2_28_sqr(const fp2_28& a) {
  fp2_28 r;
  r.c0 = fp28_mulx(fp28_add(a.c0, a.c1), fp28_sub<C, S>(a.c0, a.c1));
  r.c1 = fp28_mulx(fp28_muls<2>(a.c0), a.c1);
  return r;
}
// (both reductions always: a branch between them would merge the limbs' register pairs of the two
// paths and lose that their high words are zero, which the products after it pay for)
LB_HD bool fp2_28_is_zero(const fp2_28& a) { return fp28_is_zero(a.c0) & fp28_is_zero(a.c1); }
LB_HD fp2_28 fp2_28_from_fp2(const fp2& a) { return fp2_28{fp28_from_fp(a.c0), fp28_from_fp(a.c1)}; }
LB_HD fp2_28 fp2_28_from_fp2_shift(const fp2& a) { return fp2_28{fp28_from_fp_shift(a.c0), fp28_from_fp_shift(a.c1)}; }
LB_HD fp2 fp2_28_to_fp2(const fp2_28& a) { return fp2{fp28_to_fp(a.c0), fp28_to_fp(a.c1)}; }

// ---- Fp6 = Fp2[v] / (v^3 - xi), xi = 1 + u, and the sparse Fp12 products of the Miller loop on
// the form above (k_miller_lane, lb_pairing.h).  The products read their operands coefficient by
// coefficient through a(i), b(i) and hand each finished coefficient to out(i, .), so a caller
// whose Fp6 values live in memory slots never holds a whole one in registers: operand sums are
// formed where they are used and a result goes straight to its slot.  Every out() value is
// normalised.  The template constants are the C of each subtraction (its S is fixed by the limb
// bound written beside it); the call sites in lb_pairing.h give the values they are sized for.
struct fp6_28 {
  fp2_28 c0, c1, c2;
};
// a xi = (a0 - a1) + (a0 + a1) u: one a + K - b and one limb-wise add
template <uint32_t C, int S>
LB_HD fp2_28 fp2_28_mul_xi(const fp2_28& a) {
  return fp2_28{fp28_sub<C, S>(a.c0, a.c1), fp28_add(a.c0, a.c1)};
}
template <uint32_t C, int S>
LB_HD fp2_28 fp2_28_kminus(const fp2_28& a) {
  return fp2_28{fp28_kminus<C, S>(a.c0), fp28_kminus<C, S>(a.c1)};
}
LB_HD fp6_28 fp6_28_add(const fp6_28& a, const fp6_28& b) {
  return fp6_28{fp2_28_add(a.c0, b.c0), fp2_28_add(a.c1, b.c1), fp2_28_add(a.c2, b.c2)};
}
template <uint32_t C, int S>
LB_HD fp6_28 fp6_28_sub(const fp6_28& a, const fp6_28& b) {
  return fp6_28{fp2_28_sub<C, S>(a.c0, b.c0), fp2_28_sub<C, S>(a.c1, b.c1), fp2_28_sub<C, S>(a.c2, b.c2)};
}
template <uint32_t C, int S>  // a v = (xi a2, a0, a1)
LB_HD fp6_28 fp6_28_mul_v(const fp6_28& a) {
  return fp6_28{fp2_28_mul_xi<C, S>(a.c2), a.c0, a.c1};
}
LB_HD fp6_28 fp6_28_norm(const fp6_28& a) { return fp6_28{fp2_28_norm(a.c0), fp2_28_norm(a.c1), fp2_28_norm(a.c2)}; }
// Karatsuba a b (the product tree of fp6_mul_inl), a(i), b(i) normalised and none of them written
// by out.  CB covers one coefficient of b, CB2 the sum of two, CT the sum of two of t0..t2, CX
// m12 + K - (t1 + t2), CXT one of t0..t2.  6 products, 6 fp2_28_norm.
template <uint32_t CB, uint32_t CB2, uint32_t CT, uint32_t CX, uint32_t CXT, class A, class B, class O>
LB_HD void fp6_28_mul_to(A&& a, B&& b, O&& out) {
  const fp2_28 t0 = fp2_28_mul<CB, 28>(a(0), b(0));
  const fp2_28 t1 = fp2_28_mul<CB, 28>(a(1), b(1));
  const fp2_28 t2 = fp2_28_mul<CB, 28>(a(2), b(2));
  {  // c0 = xi ((a1 + a2)(b1 + b2) - t1 - t2) + t0: sums' limbs 2^29; x's 4 x 2^28; xi x's 13 x 2^28
    const fp2_28 m = fp2_28_mul<CB2, 29>(fp2_28_add(a(1), a(2)), fp2_28_add(b(1), b(2)));
    const fp2_28 x = fp2_28_sub<CT, 29>(m, fp2_28_add(t1, t2));
    out(0, fp2_28_norm(fp2_28_add(fp2_28_mul_xi<CX, 31>(x), t0)));
  }
  {  // c1 = (a0 + a1)(b0 + b1) - t0 - t1 + xi t2
    const fp2_28 m = fp2_28_mul<CB2, 29>(fp2_28_add(a(0), a(1)), fp2_28_add(b(0), b(1)));
    out(1, fp2_28_norm(fp2_28_add(fp2_28_sub<CT, 29>(m, fp2_28_add(t0, t1)), fp2_28_mul_xi<CXT, 28>(t2))));
  }
  {  // c2 = (a0 + a2)(b0 + b2) - t0 - t2 + t1
    const fp2_28 m = fp2_28_mul<CB2, 29>(fp2_28_add(a(0), a(2)), fp2_28_add(b(0), b(2)));
    out(2, fp2_28_norm(fp2_28_add(fp2_28_sub<CT, 29>(m, fp2_28_add(t0, t2)), t1)));
  }
}
// a (b0 + b1 v) (fp6_mul_01), bs = b0 + b1; b0, b1, bs normalised, a's limbs up to 2^29.  out may
// write the slot a is read from: a(0), a(1) are read before the first out, a(2) after out(1) only.
// CB0, CB1, CBS cover b0, b1, bs; CT covers t0 + t1; CX covers a2 b1.  5 products, 3 fp2_28_norm.
template <uint32_t CB0, uint32_t CB1, uint32_t CBS, uint32_t CT, uint32_t CX, class A, class O>
LB_HD void fp6_28_mul_01_to(A&& a, const fp2_28& b0, const fp2_28& b1, const fp2_28& bs, O&& out) {
  const fp2_28 t0 = fp2_28_mul<CB0, 28>(a(0), b0);
  const fp2_28 t1 = fp2_28_mul<CB1, 28>(a(1), b1);
  out(1, fp2_28_norm(fp2_28_sub<CT, 29>(fp2_28_mul<CBS, 28>(fp2_28_add(a(0), a(1)), bs), fp2_28_add(t0, t1))));
  out(0, fp2_28_norm(fp2_28_add(fp2_28_mul_xi<CX, 28>(fp2_28_mul<CB1, 28>(a(2), b1)), t0)));
  out(2, fp2_28_add(fp2_28_mul<CB0, 28>(a(2), b0), t1));  // limbs below 2^29: the callers add and normalise
}
// a (b1 v) (fp6_mul_1): 3 products, 1 fp2_28_norm
template <uint32_t CB1, uint32_t CX, class A, class O>
LB_HD void fp6_28_mul_1_to(A&& a, const fp2_28& b1, O&& out) {
  out(0, fp2_28_norm(fp2_28_mul_xi<CX, 28>(fp2_28_mul<CB1, 28>(a(2), b1))));
  out(1, fp2_28_mul<CB1, 28>(a(0), b1));
  out(2, fp2_28_mul<CB1, 28>(a(1), b1));
}
// fp6_28_at: coefficient i of a value; the kernel's step functions collect a product's output in one.
// The whole-value forms after it (fp6_28_mul, _mul_01, _mul_1, and fp6_28_add / _sub / _mul_v / _norm
// above) are host-check helpers: tests/native/miller28_check.cpp compares them with the 12-word tower
// at the call sites' bounds.  No kernel calls them; the kernels go through the _to forms.
LB_HD const fp2_28& fp6_28_at(const fp6_28& a, int i) { return i == 0 ? a.c0 : i == 1 ? a.c1 : a.c2; }
LB_HD fp2_28& fp6_28_at(fp6_28& a, int i) { return i == 0 ? a.c0 : i == 1 ? a.c1 : a.c2; }
template <uint32_t CB, uint32_t CB2, uint32_t CT, uint32_t CX, uint32_t CXT>
LB_HD fp6_28 fp6_28_mul(const fp6_28& a, const fp6_28& b) {
  fp6_28 r;
  fp6_28_mul_to<CB, CB2, CT, CX, CXT>([&](int i) { return fp6_28_at(a, i); }, [&](int i) { return fp6_28_at(b, i); },
                                      [&](int i, const fp2_28& v) { fp6_28_at(r, i) = v; });
  return r;
}
template <uint32_t CB0, uint32_t CB1, uint32_t CBS, uint32_t CT, uint32_t CX>
LB_HD fp6_28 fp6_28_mul_01(const fp6_28& a, const fp2_28& b0, const fp2_28& b1) {
  fp6_28 r;
  fp6_28_mul_01_to<CB0, CB1, CBS, CT, CX>([&](int i) { return fp6_28_at(a, i); }, b0, b1, fp2_28_norm(fp2_28_add(b0, b1)),
                                          [&](int i, const fp2_28& v) { fp6_28_at(r, i) = v; });
  return r;
}
template <uint32_t CB1, uint32_t CX>
LB_HD fp6_28 fp6_28_mul_1(const fp6_28& a, const fp2_28& b1) {
  fp6_28 r;
  fp6_28_mul_1_to<CB1, CX>([&](int i) { return fp6_28_at(a, i); }, b1, [&](int i, const fp2_28& v) { fp6_28_at(r, i) = v; });
  return r;
}

template <bool kInlMul = false>
LB_HD fp fp_pow_const_i(fp a, const uint32_t* e, int top_bit) {
  if constexpr (kInlMul) return fp_pow_const_28(a, e, top_bit);
  fp tab[8];
  tab[0] = a;
  const fp a2 = fp_sqr(a);
  LB_UNROLL for (int k = 1; k < 8; k++) tab[k] = fp_mul(tab[k - 1], a2);
  auto bit = [&](int i) -> uint32_t { return (e[i >> 5] >> (i & 31)) & 1u; };
  fp r = fp_zero();
  bool first = true;
  int i = top_bit;
  while (i >= 0) {
    if (!bit(i)) {
      r = fp_sqr(r);
      i--;
      continue;
    }
    int j = i - 3 > 0 ? i - 3 : 0;
    while (!bit(j)) j++;
    uint32_t val = 0;
    for (int k = i; k >= j; k--) val = (val << 1) | bit(k);
    if (first) {
      r = lb_tab8(tab, val >> 1);
      first = false;
    } else {
      for (int k = i; k >= j; k--) r = fp_sqr(r);
      r = fp_mul(r, lb_tab8(tab, val >> 1));
    }
    i = j - 1;
  }
  return r;
}

// ---- word-array helpers of the variable-time algorithms below (the safegcd inversion, the binary
// Jacobi symbol).  Every value this engine inverts or tests is derived from public data
// (signatures, pubkeys, messages), so timing does not leak secrets.
LB_HD bool lb_is_one_plain(const uint32_t* x) {
  uint32_t t = x[0] ^ 1u;
  LB_UNROLL for (int i = 1; i < 12; i++) t |= x[i];
  return t == 0;
}
LB_HD int lb_ctz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_ctz(x);
#else
  return __builtin_ctz(x);
#endif
}
// u <- u / 2^k (plain shift), 1 <= k <= 31
LB_HD void lb_shr(uint32_t* u, int k) {
  LB_UNROLL for (int j = 0; j < 11; j++) u[j] = (u[j] >> k) | (u[j + 1] << (32 - k));
  u[11] >>= k;
}
LB_HD bool lb_geq(const uint32_t* a, const uint32_t* b) {
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) (void)LB_SUBC(a[j], b[j], br, &br);
  return br == 0;
}
LB_HD void lb_sub_in(uint32_t* a, const uint32_t* b) {
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) a[j] = LB_SUBC(a[j], b[j], br, &br);
}
// ---- Bernstein-Yang "safegcd" inversion, variable time (jumps of 62 divsteps on the low 64 bits,
// then 2x2 transition matrices applied to the full-width values; the divstep loop and the
// update steps follow the structure of libsecp256k1's modinv64_var, written here for a 381-bit
// modulus in 7 signed 62-bit limbs).  ~12 jumps for a random input against the binary extended
// Euclid's ~760 word-array iterations: an inversion on a lone lane 184 us -> ~25 us
// (tools/ubench/row_bench.hip), on the critical path of every small batch (the final
// exponentiation's norm, each block's batched inversion in k_hash_finish / k_gsum_final /
// k_pk_blind, ML(-G1, S)'s affine S).  Public inputs only, so variable time is fine.
struct lb_s62 {
  int64_t v[7];
};
#define LB_S62_M 0x3fffffffffffffffLL
LB_HD lb_s62 lb_s62_p() {
  return lb_s62{{0x39feffffffffaaabLL, 0x3aaffffac54ffffeLL, 0x330d2a0f6b0f6241LL, 0x1dd2e13ce144afd9LL,
                 0x1ba7b6434bacd764LL, 0x0447a8e5ff9a692cLL, 0x1a0LL}};
}
#define LB_S62_PINV 0x360c000300030003ULL  // p^-1 mod 2^62
LB_HD int lb_ctz64(uint64_t x) { return __builtin_ctzll(x); }
// 62 divsteps on the low bits of f, g (f odd); returns the new eta, the matrix in t[4] = u, v, q, r
LB_HD int64_t lb_divsteps62(int64_t eta, uint64_t f0, uint64_t g0, int64_t t[4]) {
  uint64_t u = 1, v = 0, q = 0, r = 1, f = f0, g = g0, m, w;
  int i = 62;
  for (;;) {
    const int zeros = lb_ctz64(g | (~0ULL << i));  // sentinel at bit i
    g >>= zeros;
    u <<= zeros;
    v <<= zeros;
    eta -= zeros;
    i -= zeros;
    if (i == 0) break;
    int limit;
    if (eta < 0) {  // swap with negation: (f, g) <- (g, -f)
      uint64_t tmp;
      eta = -eta;
      tmp = f; f = g; g = (uint64_t)0 - tmp;
      tmp = u; u = q; q = (uint64_t)0 - tmp;
      tmp = v; v = r; r = (uint64_t)0 - tmp;
      limit = (int)eta + 1 > i ? i : (int)eta + 1;
      m = (~0ULL >> (64 - limit)) & 63u;
      w = (f * g * (f * f - 2)) & m;  // cancels up to 6 low bits of g
    } else {
      limit = (int)eta + 1 > i ? i : (int)eta + 1;
      m = (~0ULL >> (64 - limit)) & 15u;
      w = f + (((f + 1) & 4) << 1);
      w = ((uint64_t)0 - w * g) & m;  // up to 4 bits
    }
    g += f * w;
    q += u * w;
    r += v * w;
  }
  t[0] = (int64_t)u;
  t[1] = (int64_t)v;
  t[2] = (int64_t)q;
  t[3] = (int64_t)r;
  return eta;
}
// (f, g) <- (u f + v g, q f + r g) / 2^62 (exact)
LB_HD void lb_s62_update_fg(lb_s62& f, lb_s62& g, const int64_t t[4]) {
  const int64_t u = t[0], v = t[1], q = t[2], r = t[3];
  __int128 cf = (__int128)u * f.v[0] + (__int128)v * g.v[0];
  __int128 cg = (__int128)q * f.v[0] + (__int128)r * g.v[0];
  cf >>= 62;
  cg >>= 62;
  LB_UNROLL for (int i = 1; i < 7; i++) {
    cf += (__int128)u * f.v[i] + (__int128)v * g.v[i];
    cg += (__int128)q * f.v[i] + (__int128)r * g.v[i];
    f.v[i - 1] = (int64_t)cf & LB_S62_M;
    cf >>= 62;
    g.v[i - 1] = (int64_t)cg & LB_S62_M;
    cg >>= 62;
  }
  f.v[6] = (int64_t)cf;
  g.v[6] = (int64_t)cg;
}
// (d, e) <- (u d + v e, q d + r e) / 2^62 mod p, kept in (-2p, p)
LB_HD void lb_s62_update_de(lb_s62& d, lb_s62& e, const int64_t t[4]) {
  const lb_s62 M = lb_s62_p();
  const int64_t u = t[0], v = t[1], q = t[2], r = t[3];
  const int64_t sd = d.v[6] >> 63, se = e.v[6] >> 63;
  int64_t md = (u & sd) + (v & se), me = (q & sd) + (r & se);
  __int128 cd = (__int128)u * d.v[0] + (__int128)v * e.v[0];
  __int128 ce = (__int128)q * d.v[0] + (__int128)r * e.v[0];
  md -= (int64_t)((LB_S62_PINV * (uint64_t)cd + (uint64_t)md) & (uint64_t)LB_S62_M);
  me -= (int64_t)((LB_S62_PINV * (uint64_t)ce + (uint64_t)me) & (uint64_t)LB_S62_M);
  cd += (__int128)M.v[0] * md;
  ce += (__int128)M.v[0] * me;
  cd >>= 62;
  ce >>= 62;
  LB_UNROLL for (int i = 1; i < 7; i++) {
    cd += (__int128)u * d.v[i] + (__int128)v * e.v[i] + (__int128)M.v[i] * md;
    ce += (__int128)q * d.v[i] + (__int128)r * e.v[i] + (__int128)M.v[i] * me;
    d.v[i - 1] = (int64_t)cd & LB_S62_M;
    cd >>= 62;
    e.v[i - 1] = (int64_t)ce & LB_S62_M;
    ce >>= 62;
  }
  d.v[6] = (int64_t)cd;
  e.v[6] = (int64_t)ce;
}
// r in (-2p, p) -> r * sign (sign = +-1 as the sign of the top limb of f) in [0, p)
LB_HD void lb_s62_normalize(lb_s62& r, int64_t sign) {
  const lb_s62 M = lb_s62_p();
  int64_t cond = r.v[6] >> 63;
  LB_UNROLL for (int i = 0; i < 7; i++) r.v[i] += M.v[i] & cond;
  const int64_t neg = sign >> 63;
  LB_UNROLL for (int i = 0; i < 7; i++) r.v[i] = (r.v[i] ^ neg) - neg;
  LB_UNROLL for (int i = 0; i < 6; i++) {
    r.v[i + 1] += r.v[i] >> 62;
    r.v[i] &= LB_S62_M;
  }
  cond = r.v[6] >> 63;
  LB_UNROLL for (int i = 0; i < 7; i++) r.v[i] += M.v[i] & cond;
  LB_UNROLL for (int i = 0; i < 6; i++) {
    r.v[i + 1] += r.v[i] >> 62;
    r.v[i] &= LB_S62_M;
  }
}
LB_HD uint64_t lb_bits64(const uint32_t* w, int off, int nbits) {  // bits [off, off + nbits) of 12 words
  const int q = off >> 5, s = off & 31;
  uint64_t x = 0;
  LB_UNROLL for (int k = 0; k < 3; k++) {
    const int j = q + k;
    const uint64_t wj = j < 12 ? w[j] : 0u;
    if (k == 0) x = wj >> s;
    else x |= (32 * k - s) < 64 ? wj << (32 * k - s) : 0;
  }
  return nbits >= 64 ? x : (x & ((1ULL << nbits) - 1));
}
// The Jacobi symbol by "posdivsteps" (the Jacobi variant of the divsteps above, as in
// libsecp256k1's modinv64 jacobi): f, g stay non-negative (a swap does not negate), and the
// symbol's sign bit in jac flips when g loses an odd power of 2 while f = 3, 5 mod 8, and when a
// swap meets f = g = 3 mod 4.  ~20 jumps of 62 steps against the binary algorithm's ~760
// word-array iterations (hash_to_G2's is_square: ~184 us -> tens of us on a lone lane).
LB_HD int64_t lb_posdivsteps62(int64_t eta, uint64_t f0, uint64_t g0, int64_t t[4], int& jac) {
  uint64_t u = 1, v = 0, q = 0, r = 1, f = f0, g = g0, m, w;
  int i = 62;
  for (;;) {
    const int zeros = lb_ctz64(g | (~0ULL << i));
    g >>= zeros;
    u <<= zeros;
    v <<= zeros;
    eta -= zeros;
    i -= zeros;
    jac ^= (int)(zeros & ((f >> 1) ^ (f >> 2)));
    if (i == 0) break;
    int limit;
    if (eta < 0) {  // swap (no negation)
      uint64_t tmp;
      eta = -eta;
      tmp = f; f = g; g = tmp;
      tmp = u; u = q; q = tmp;
      tmp = v; v = r; r = tmp;
      jac ^= (int)((f & g) >> 1);
      limit = (int)eta + 1 > i ? i : (int)eta + 1;
      m = (~0ULL >> (64 - limit)) & 63u;
      w = (f * g * (f * f - 2)) & m;
    } else {
      limit = (int)eta + 1 > i ? i : (int)eta + 1;
      m = (~0ULL >> (64 - limit)) & 15u;
      w = f + (((f + 1) & 4) << 1);
      w = ((uint64_t)0 - w * g) & m;
    }
    g += f * w;
    q += u * w;
    r += v * w;
  }
  t[0] = (int64_t)u;
  t[1] = (int64_t)v;
  t[2] = (int64_t)q;
  t[3] = (int64_t)r;
  return eta;
}
// (x | p) for x in [0, p) given as 12 words (0 counts as a square): 1 square, 0 non-square,
// -1 not settled within the jump budget (the caller falls back to the binary algorithm)
LB_HD int fp_is_square_sg(const fp& x) {
  if (fp_is_zero(x)) return 1;
  lb_s62 f = lb_s62_p(), g;
  LB_UNROLL for (int i = 0; i < 7; i++) g.v[i] = (int64_t)lb_bits64(x.v, 62 * i, 62);
  int64_t eta = -1, t[4];
  int jac = 0;
  for (int it = 0; it < 60; it++) {
    // 64 low bits (the symbol's updates read f mod 8 up to the 62nd step)
    eta = lb_posdivsteps62(eta, (uint64_t)f.v[0] | ((uint64_t)f.v[1] << 62), (uint64_t)g.v[0] | ((uint64_t)g.v[1] << 62),
                           t, jac);
    lb_s62_update_fg(f, g, t);
    if (f.v[0] == 1) {
      int64_t any = 0;
      LB_UNROLL for (int i = 1; i < 7; i++) any |= f.v[i];
      if (any == 0) return (jac & 1) ? 0 : 1;
    }
  }
  return -1;
}
// plain a in [0, p) -> a^-1 mod p (plain), 0 -> 0
LB_HD fp fp_inv_plain_by_i(const fp& a) {
  if (fp_is_zero(a)) return a;
  lb_s62 f = lb_s62_p(), g, d, e;
  LB_UNROLL for (int i = 0; i < 7; i++) {
    g.v[i] = (int64_t)lb_bits64(a.v, 62 * i, 62);
    d.v[i] = 0;
    e.v[i] = i == 0;
  }
  int64_t eta = -1, t[4];
  for (int it = 0; it < 40; it++) {  // (a 381-bit modulus needs <= 18 jumps)
    eta = lb_divsteps62(eta, (uint64_t)f.v[0], (uint64_t)g.v[0], t);
    lb_s62_update_de(d, e, t);
    lb_s62_update_fg(f, g, t);
    if (g.v[0] == 0) {
      int64_t any = 0;
      LB_UNROLL for (int i = 1; i < 7; i++) any |= g.v[i];
      if (any == 0) break;
    }
  }
  lb_s62_normalize(d, f.v[6]);  // f = +-1: the sign of its top limb
  fp r;
  LB_UNROLL for (int w = 0; w < 12; w++) {
    const int b = 32 * w, i = b / 62, sft = b - 62 * i;
    uint64_t x = (uint64_t)d.v[i] >> sft;
    if (i + 1 < 7 && sft > 30) x |= (uint64_t)d.v[i + 1] << (62 - sft);
    r.v[w] = (uint32_t)x;
  }
  return r;
}
// plain a in [0, p) -> a^-1 mod p (plain), 0 -> 0: the out-of-line entry (fp_inv_plain_by_i is the
// inline body: a kernel whose call graph is all inline keeps its own register budget)
LB_NI fp fp_inv_plain_vt(fp a) { return fp_inv_plain_by_i(a); }
// Montgomery a R -> a^-1 R:  plain inverse of (a R) is a^-1 R^-1; times R^3 / R gives a^-1 R
LB_HD fp fp_inv(const fp& a) { return fp_mul(fp_inv_plain_vt(a), fp_load(LB_R3)); }  // inv(0)=0
LB_HD fp fp_inv_i(const fp& a) {
  return fp_mul(fp_inv_plain_by_i(a), fp_load(LB_R3));
}
LB_NI fp fp_pow_const(fp a, const uint32_t* e, int top_bit) { return fp_pow_const_i<true>(a, e, top_bit); }
LB_HD fp fp_sqrt_cand(const fp& a) { return fp_pow_const(a, LB_EXP_SQRT, 378); }   // a^((p+1)/4)
LB_HD fp fp_isqrt_cand(const fp& a) { return fp_pow_const(a, LB_EXP_ISQRT, 378); }  // a^((p-3)/4)
// Quadratic character by the binary Jacobi-symbol algorithm (variable time; every input is
// public: SSWU on hashed messages).  Works on the Montgomery representation directly:
// (aR / p) = (a / p) (R / p) and R = 2^384 is a square.  ~400 shift/subtract steps instead of
// the 570-multiplication Legendre exponentiation a^((p-1)/2).
LB_NI bool fp_is_square(fp a) {
  if (fp_is_zero(a)) return true;
  uint32_t u[12], v[12];
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  LB_UNROLL for (int j = 0; j < 12; j++) {
    u[j] = a.v[j];
    v[j] = Pl[j];
  }
  int t = 1;  // (u / v) * t is the answer; v stays odd
  while (true) {
    // remove factors of two from u: (2 / v) = -1 iff v = 3, 5 (mod 8)
    while (u[0] == 0) {
      LB_UNROLL for (int j = 0; j < 11; j++) u[j] = u[j + 1];
      u[11] = 0;  // 2^32 is a square: no sign change
    }
    int k = lb_ctz32(u[0]);
    if (k) {
      lb_shr(u, k);
      uint32_t v8 = v[0] & 7u;
      if ((k & 1) && (v8 == 3u || v8 == 5u)) t = -t;
    }
    if (lb_is_one_plain(u)) return t == 1;
    // both odd: make u >= v by swapping (quadratic reciprocity), then u -= v
    if (!lb_geq(u, v)) {
      if ((u[0] & 3u) == 3u && (v[0] & 3u) == 3u) t = -t;
      LB_UNROLL for (int j = 0; j < 12; j++) {
        uint32_t x = u[j];
        u[j] = v[j];
        v[j] = x;
      }
      if (lb_is_one_plain(u)) return t == 1;
    }
    lb_sub_in(u, v);
    bool zero = true;
    LB_UNROLL for (int j = 0; j < 12; j++) zero &= u[j] == 0;
    if (zero) return false;  // gcd > 1 cannot happen for prime p and a != 0
  }
}

// canonical (non-Montgomery) value compared with (p-1)/2: returns a > (p-1)/2
LB_HD bool fp_plain_gt_half(const fp& plain) {
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) {
    uint64_t d = (uint64_t)LB_HALF_P[j] - plain.v[j] - br;
    br = (uint32_t)(d >> 63);
  }
  return br != 0;  // half - a < 0
}

// 48-byte big-endian -> plain limbs; returns false if value >= p (blst BAD_ENCODING)
LB_HD bool fp_plain_from_be48(fp& out, const uint8_t* b, uint8_t first_byte_mask) {
  LB_UNROLL for (int i = 0; i < 12; i++) {
    int o = 44 - 4 * i;
    uint32_t b0 = b[o];
    if (i == 11) b0 &= first_byte_mask;
    out.v[i] = (b0 << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | b[o + 3];
  }
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) {
    uint64_t d = (uint64_t)out.v[j] - Pl[j] - br;
    br = (uint32_t)(d >> 63);
  }
  return br != 0;  // out < p
}

// the same from 12 little-endian-loaded words of the 48 bytes (w[k] = bytes 4k..4k+3): no byte
// buffer, so a kernel keeps the encoding in registers
LB_HD uint32_t lb_bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }
LB_HD bool fp_plain_from_be48_w(fp& out, const uint32_t* w, uint8_t first_byte_mask) {
  LB_UNROLL for (int i = 0; i < 12; i++) out.v[i] = lb_bswap32(w[11 - i]);
  out.v[11] &= ((uint32_t)first_byte_mask << 24) | 0x00ffffffu;
  const uint32_t Pl[12] = {LB_P0, LB_P1, LB_P2, LB_P3, LB_P4, LB_P5, LB_P6, LB_P7, LB_P8, LB_P9, LB_P10, LB_P11};
  uint32_t br = 0;
  LB_UNROLL for (int j = 0; j < 12; j++) {
    uint64_t d = (uint64_t)out.v[j] - Pl[j] - br;
    br = (uint32_t)(d >> 63);
  }
  return br != 0;  // out < p
}

LB_HD void fp_plain_to_be48(uint8_t* b, const fp& plain) {
  LB_UNROLL for (int i = 0; i < 12; i++) {
    int o = 44 - 4 * i;
    uint32_t w = plain.v[i];
    b[o] = (uint8_t)(w >> 24);
    b[o + 1] = (uint8_t)(w >> 16);
    b[o + 2] = (uint8_t)(w >> 8);
    b[o + 3] = (uint8_t)w;
  }
}

// ------------------------------------------------------------------ Fp2
LB_HD fp2 fp2_zero() { return fp2{fp_zero(), fp_zero()}; }
LB_HD fp2 fp2_one() { return fp2{fp_one(), fp_zero()}; }
LB_HD bool fp2_is_zero(const fp2& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
LB_HD bool fp2_eq(const fp2& a, const fp2& b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }
LB_HD fp2 fp2_select(bool c, const fp2& a, const fp2& b) { return fp2{fp_select(c, a.c0, b.c0), fp_select(c, a.c1, b.c1)}; }
LB_HD fp2 fp2_add(const fp2& a, const fp2& b) { return fp2{fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
LB_HD fp2 fp2_sub(const fp2& a, const fp2& b) { return fp2{fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)}; }
LB_HD fp2 fp2_dbl(const fp2& a) { return fp2{fp_dbl(a.c0), fp_dbl(a.c1)}; }
LB_HD fp2 fp2_neg(const fp2& a) { return fp2{fp_neg(a.c0), fp_neg(a.c1)}; }
LB_HD fp2 fp2_conj(const fp2& a) { return fp2{a.c0, fp_neg(a.c1)}; }
LB_HD fp2 fp2_mul_fp(const fp2& a, const fp& s) { return fp2{fp_mul(a.c0, s), fp_mul(a.c1, s)}; }
LB_HD fp2 fp2_mul3(const fp2& a) { return fp2{fp_mul3(a.c0), fp_mul3(a.c1)}; }
LB_HD fp2 fp2_mul4(const fp2& a) { return fp2{fp_mul4(a.c0), fp_mul4(a.c1)}; }
LB_HD fp2 fp2_mul8(const fp2& a) { return fp2{fp_mul8(a.c0), fp_mul8(a.c1)}; }

// Fp2 arithmetic is inline (its three products are calls to fp_mul); the Fp6 / Fp12 layers
// and the group law are out of line with pointer / by-value arguments.
LB_HD fp2 fp2_mul(const fp2& a, const fp2& b) {
  fp t0 = fp_mul(a.c0, b.c0);
  fp t1 = fp_mul(a.c1, b.c1);
  fp t2 = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
  return fp2{fp_sub(t0, t1), fp_sub(fp_sub(t2, t0), t1)};
}
LB_HD fp2 fp2_sqr(const fp2& a) {
  fp t0 = fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1));
  fp t1 = fp_mul(a.c0, a.c1);
  return fp2{t0, fp_dbl(t1)};
}
// multiply by the non-residue xi = 1 + u
LB_HD fp2 fp2_mul_xi(const fp2& a) { return fp2{fp_sub(a.c0, a.c1), fp_add(a.c0, a.c1)}; }

LB_NI fp2 fp2_inv(fp2 a) {
  fp n = fp_add(fp_sqr(a.c0), fp_sqr(a.c1));
  fp ni = fp_inv(n);
  return fp2{fp_mul(a.c0, ni), fp_neg(fp_mul(a.c1, ni))};
}

LB_HD bool fp2_is_square(const fp2& a) { return fp_is_square(fp_add(fp_sqr(a.c0), fp_sqr(a.c1))); }

// Square root in Fp2 by the complex method (p = 3 mod 4): three Fp exponentiations,
// no data-dependent branches.  Returns true iff a is a square; `out` is some root.
// fp2_sqrt_i is the inline body (signature decoding keeps its point in registers), fp2_sqrt
// the out-of-line entry.
template <bool kInl = false>
LB_HD bool fp2_sqrt_i(fp2& out, const fp2& a) {
  fp norm = fp_add(fp_sqr(a.c0), fp_sqr(a.c1));
  fp alpha;
  if constexpr (kInl) alpha = fp_pow_const_i<true>(norm, LB_EXP_SQRT, 378);
  else alpha = fp_sqrt_cand(norm);  // sqrt(norm) if it exists
  fp inv2 = fp_load(LB_INV2);
  fp d1 = fp_mul(fp_add(a.c0, alpha), inv2);
  fp d2 = fp_mul(fp_sub(a.c0, alpha), inv2);
  // (a0 + alpha)/2 is zero only when a1 == 0 and alpha == -a0; use the other candidate
  fp delta = fp_select(fp_is_zero(d1), d2, d1);
  // z = delta^((p-3)/4), s = delta z = delta^((p+1)/4), and s z = delta^((p-1)/2) = +-1, so
  // 1/s = +-z: the square root and the inverse it needs come from one exponentiation
  fp z;
  if constexpr (kInl) z = fp_pow_const_i<true>(delta, LB_EXP_ISQRT, 378);
  else z = fp_isqrt_cand(delta);
  fp s = fp_mul(delta, z);
  bool delta_qr = fp_eq(fp_sqr(s), delta);
  // if delta is a residue: x0 = s, x1 = a1/(2s); else (s^2 = -delta) x0 = a1/(2s), x1 = s
  fp t = fp_mul(z, inv2);
  if (!delta_qr) t = fp_neg(t);
  fp q = fp_mul(a.c1, t);
  out.c0 = fp_select(delta_qr, s, q);
  out.c1 = fp_select(delta_qr, q, s);
  return fp2_eq(fp2_sqr(out), a);
}
LB_NI bool fp2_sqrt(fp2& out, fp2 a) { return fp2_sqrt_i(out, a); }
// the same with the two exponentiations by pow(x, exponent words, top bit) (k_hash_map_row: on a row)
template <class Pow>
LB_HD bool fp2_sqrt_p(fp2& out, const fp2& a, Pow pow) {
  const fp norm = fp_add(fp_sqr(a.c0), fp_sqr(a.c1));
  const fp alpha = pow(norm, LB_EXP_SQRT, 378);
  const fp inv2 = fp_load(LB_INV2);
  const fp d1 = fp_mul(fp_add(a.c0, alpha), inv2);
  const fp d2 = fp_mul(fp_sub(a.c0, alpha), inv2);
  const fp delta = fp_select(fp_is_zero(d1), d2, d1);
  const fp z = pow(delta, LB_EXP_ISQRT, 378);
  const fp s = fp_mul(delta, z);
  const bool delta_qr = fp_eq(fp_sqr(s), delta);
  fp t = fp_mul(z, inv2);
  if (!delta_qr) t = fp_neg(t);
  const fp q = fp_mul(a.c1, t);
  out.c0 = fp_select(delta_qr, s, q);
  out.c1 = fp_select(delta_qr, q, s);
  return fp2_eq(fp2_sqr(out), a);
}

// RFC 9380 sgn0 for Fp2 (on canonical values)
LB_HD uint32_t fp2_sgn0(const fp2& a) {
  fp p0 = fp_from_mont(a.c0), p1 = fp_from_mont(a.c1);
  uint32_t sign0 = p0.v[0] & 1u;
  uint32_t zero0 = fp_is_zero(p0) ? 1u : 0u;
  uint32_t sign1 = p1.v[0] & 1u;
  return sign0 | (zero0 & sign1);
}

// ZCash "lexicographically largest" for Fp2: decided by c1 unless c1 == 0
LB_HD bool fp2_lex_larger(const fp2& a) {
  fp p0 = fp_from_mont(a.c0), p1 = fp_from_mont(a.c1);
  return fp_is_zero(p1) ? fp_plain_gt_half(p0) : fp_plain_gt_half(p1);
}

// ------------------------------------------------------------------ Fp6
LB_HD fp6 fp6_zero() { return fp6{fp2_zero(), fp2_zero(), fp2_zero()}; }
LB_HD fp6 fp6_one() { return fp6{fp2_one(), fp2_zero(), fp2_zero()}; }
LB_HD fp6 fp6_add(const fp6& a, const fp6& b) { return fp6{fp2_add(a.c0, b.c0), fp2_add(a.c1, b.c1), fp2_add(a.c2, b.c2)}; }
LB_HD fp6 fp6_sub(const fp6& a, const fp6& b) { return fp6{fp2_sub(a.c0, b.c0), fp2_sub(a.c1, b.c1), fp2_sub(a.c2, b.c2)}; }
LB_HD fp6 fp6_neg(const fp6& a) { return fp6{fp2_neg(a.c0), fp2_neg(a.c1), fp2_neg(a.c2)}; }
LB_HD fp6 fp6_mul_v(const fp6& a) { return fp6{fp2_mul_xi(a.c2), a.c0, a.c1}; }

// Inline body (the Miller loop kernel keeps its Fp12 state in registers); fp6_mul_p is the
// out-of-line entry everything else calls.
LB_HD fp6 fp6_mul_inl(const fp6& a, const fp6& b) {
  fp2 t0 = fp2_mul(a.c0, b.c0);
  fp2 t1 = fp2_mul(a.c1, b.c1);
  fp2 t2 = fp2_mul(a.c2, b.c2);
  fp2 c0 = fp2_add(fp2_mul_xi(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c1, a.c2), fp2_add(b.c1, b.c2)), t1), t2)), t0);
  fp2 c1 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c0, a.c1), fp2_add(b.c0, b.c1)), t0), t1), fp2_mul_xi(t2));
  fp2 c2 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c0, a.c2), fp2_add(b.c0, b.c2)), t0), t2), t1);
  return fp6{c0, c1, c2};
}
LB_NI void fp6_mul_p(fp6* r, const fp6* pa, const fp6* pb) { *r = fp6_mul_inl(*pa, *pb); }
LB_HD fp6 fp6_mul(const fp6& a, const fp6& b) {
  fp6 r;
  fp6_mul_p(&r, &a, &b);
  return r;
}

// a * (b0 + b1 v)  (sparse: c2 coefficient zero)
LB_HD fp6 fp6_mul_01(const fp6& a, const fp2& b0, const fp2& b1) {
  fp2 t0 = fp2_mul(a.c0, b0);
  fp2 t1 = fp2_mul(a.c1, b1);
  fp2 c0 = fp2_add(fp2_mul_xi(fp2_mul(a.c2, b1)), t0);
  fp2 c1 = fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c0, a.c1), fp2_add(b0, b1)), t0), t1);
  fp2 c2 = fp2_add(fp2_mul(a.c2, b0), t1);
  return fp6{c0, c1, c2};
}

// a * (b1 v)
LB_HD fp6 fp6_mul_1(const fp6& a, const fp2& b1) {
  return fp6{fp2_mul_xi(fp2_mul(a.c2, b1)), fp2_mul(a.c0, b1), fp2_mul(a.c1, b1)};
}

LB_NI fp6 fp6_inv(fp6 a) {
  fp2 t0 = fp2_sub(fp2_sqr(a.c0), fp2_mul_xi(fp2_mul(a.c1, a.c2)));
  fp2 t1 = fp2_sub(fp2_mul_xi(fp2_sqr(a.c2)), fp2_mul(a.c0, a.c1));
  fp2 t2 = fp2_sub(fp2_sqr(a.c1), fp2_mul(a.c0, a.c2));
  fp2 d = fp2_add(fp2_mul(a.c0, t0), fp2_mul_xi(fp2_add(fp2_mul(a.c2, t1), fp2_mul(a.c1, t2))));
  fp2 di = fp2_inv(d);
  return fp6{fp2_mul(t0, di), fp2_mul(t1, di), fp2_mul(t2, di)};
}

// ------------------------------------------------------------------ Fp12
LB_HD fp12 fp12_one() { return fp12{fp6_one(), fp6_zero()}; }
LB_HD bool fp12_is_one(const fp12& a) {
  return fp2_eq(a.c0.c0, fp2_one()) && fp2_is_zero(a.c0.c1) && fp2_is_zero(a.c0.c2) && fp2_is_zero(a.c1.c0) &&
         fp2_is_zero(a.c1.c1) && fp2_is_zero(a.c1.c2);
}
LB_HD fp12 fp12_conj(const fp12& a) { return fp12{a.c0, fp6_neg(a.c1)}; }

LB_NI void fp12_mul_p(fp12* r, const fp12* pa, const fp12* pb) {
  const fp12& a = *pa;
  const fp12& b = *pb;
  fp6 t0 = fp6_mul(a.c0, b.c0);
  fp6 t1 = fp6_mul(a.c1, b.c1);
  fp6 c1 = fp6_sub(fp6_sub(fp6_mul(fp6_add(a.c0, a.c1), fp6_add(b.c0, b.c1)), t0), t1);
  fp6 c0 = fp6_add(t0, fp6_mul_v(t1));
  *r = fp12{c0, c1};
}
LB_HD fp12 fp12_mul(const fp12& a, const fp12& b) {
  fp12 r;
  fp12_mul_p(&r, &a, &b);
  return r;
}

LB_HD fp12 fp12_sqr_inl(const fp12& a) {
  // complex squaring: (a0 + a1 w)^2 = a0^2 + v a1^2 + 2 a0 a1 w
  fp6 t = fp6_mul_inl(a.c0, a.c1);
  fp6 c0 = fp6_mul_inl(fp6_add(a.c0, a.c1), fp6_add(a.c0, fp6_mul_v(a.c1)));
  c0 = fp6_sub(fp6_sub(c0, t), fp6_mul_v(t));
  return fp12{c0, fp6_add(t, t)};
}
LB_NI void fp12_sqr_p(fp12* r, const fp12* pa) { *r = fp12_sqr_inl(*pa); }
LB_HD fp12 fp12_sqr(const fp12& a) {
  fp12 r;
  fp12_sqr_p(&r, &a);
  return r;
}

// multiply by a Miller-loop line  l = (l0 + l2 v) + (l3 v) w   (w-basis: l0 w^0 + l2 w^2 + l3 w^3)
LB_HD fp12 fp12_mul_line_inl(const fp12& a, const fp2& l0, const fp2& l2, const fp2& l3) {
  fp6 t0 = fp6_mul_01(a.c0, l0, l2);
  fp6 t1 = fp6_mul_1(a.c1, l3);
  fp6 c1 = fp6_sub(fp6_sub(fp6_mul_01(fp6_add(a.c0, a.c1), l0, fp2_add(l2, l3)), t0), t1);
  fp6 c0 = fp6_add(t0, fp6_mul_v(t1));
  return fp12{c0, c1};
}
LB_NI void fp12_mul_line_p(fp12* r, const fp12* pa, const fp2* pl0, const fp2* pl2, const fp2* pl3) {
  *r = fp12_mul_line_inl(*pa, *pl0, *pl2, *pl3);
}
LB_HD fp12 fp12_mul_line(const fp12& a, const fp2& l0, const fp2& l2, const fp2& l3) {
  fp12 r;
  fp12_mul_line_p(&r, &a, &l0, &l2, &l3);
  return r;
}

LB_NI fp12 fp12_inv(fp12 a) {
  fp6 t = fp6_sub(fp6_mul(a.c0, a.c0), fp6_mul_v(fp6_mul(a.c1, a.c1)));
  fp6 ti = fp6_inv(t);
  return fp12{fp6_mul(a.c0, ti), fp6_neg(fp6_mul(a.c1, ti))};
}

// Frobenius a -> a^p.  In the w-basis a = sum a_k w^k (a_0=c0.c0, a_1=c1.c0, a_2=c0.c1,
// a_3=c1.c1, a_4=c0.c2, a_5=c1.c2), a^p = sum conj(a_k) xi^(k(p-1)/6) w^k.
LB_NI fp12 fp12_frob(fp12 a) {
  fp12 r;
  r.c0.c0 = fp2_conj(a.c0.c0);
  r.c1.c0 = fp2_mul(fp2_conj(a.c1.c0), fp2_load(LB_FROB1_1));
  r.c0.c1 = fp2_mul(fp2_conj(a.c0.c1), fp2_load(LB_FROB1_2));
  r.c1.c1 = fp2_mul(fp2_conj(a.c1.c1), fp2_load(LB_FROB1_3));
  r.c0.c2 = fp2_mul(fp2_conj(a.c0.c2), fp2_load(LB_FROB1_4));
  r.c1.c2 = fp2_mul(fp2_conj(a.c1.c2), fp2_load(LB_FROB1_5));
  return r;
}
LB_NI fp12 fp12_frob2(fp12 a) {
  fp12 r;
  r.c0.c0 = a.c0.c0;
  r.c1.c0 = fp2_mul_fp(a.c1.c0, fp_load(LB_FROB2_1));
  r.c0.c1 = fp2_mul_fp(a.c0.c1, fp_load(LB_FROB2_2));
  r.c1.c1 = fp2_mul_fp(a.c1.c1, fp_load(LB_FROB2_3));
  r.c0.c2 = fp2_mul_fp(a.c0.c2, fp_load(LB_FROB2_4));
  r.c1.c2 = fp2_mul_fp(a.c1.c2, fp_load(LB_FROB2_5));
  return r;
}

// ------------------------------------------------------------------ overloads for generic curve code
LB_HD fp f_add(const fp& a, const fp& b) { return fp_add(a, b); }
LB_HD fp f_sub(const fp& a, const fp& b) { return fp_sub(a, b); }
LB_HD fp f_mul(const fp& a, const fp& b) { return fp_mul(a, b); }
LB_HD fp f_sqr(const fp& a) { return fp_sqr(a); }
LB_HD fp f_dbl(const fp& a) { return fp_dbl(a); }
LB_HD fp f_neg(const fp& a) { return fp_neg(a); }
LB_HD fp f_mul3(const fp& a) { return fp_mul3(a); }
LB_HD fp f_mul8(const fp& a) { return fp_mul8(a); }
LB_HD fp f_inv(const fp& a) { return fp_inv(a); }
LB_HD bool f_is_zero(const fp& a) { return fp_is_zero(a); }
LB_HD bool f_eq(const fp& a, const fp& b) { return fp_eq(a, b); }
LB_HD fp f_select(bool c, const fp& a, const fp& b) { return fp_select(c, a, b); }
LB_HD void f_set_zero(fp& a) { a = fp_zero(); }
LB_HD void f_set_one(fp& a) { a = fp_one(); }

// fp with inline (fenced) products: a kernel that instantiates the generic curve code on jac<fpi>
// runs its G1 formulas without out-of-line product calls (k_pk_blind's GLV ladder)
struct fpi : fp {};
LB_HD fpi fpi_of(const fp& a) { return fpi{a}; }
LB_HD fpi f_add(const fpi& a, const fpi& b) { return fpi{fp_add(a, b)}; }
LB_HD fpi f_sub(const fpi& a, const fpi& b) { return fpi{fp_sub(a, b)}; }
LB_HD fpi f_mul(const fpi& a, const fpi& b) { return fpi{fp_mul_inl(a, b)}; }
LB_HD fpi f_sqr(const fpi& a) { return fpi{fp_sqr_inl(a)}; }
LB_HD fpi f_dbl(const fpi& a) { return fpi{fp_dbl(a)}; }
LB_HD fpi f_neg(const fpi& a) { return fpi{fp_neg(a)}; }
LB_HD fpi f_mul3(const fpi& a) { return fpi{fp_mul3(a)}; }
LB_HD fpi f_mul8(const fpi& a) { return fpi{fp_mul8(a)}; }
LB_HD bool f_is_zero(const fpi& a) { return fp_is_zero(a); }
LB_HD bool f_eq(const fpi& a, const fpi& b) { return fp_eq(a, b); }
LB_HD fpi f_select(bool c, const fpi& a, const fpi& b) { return fpi{fp_select(c, a, b)}; }
LB_HD void f_set_zero(fpi& a) { a = fpi{fp_zero()}; }
LB_HD void f_set_one(fpi& a) { a = fpi{fp_one()}; }

LB_HD fp2 f_add(const fp2& a, const fp2& b) { return fp2_add(a, b); }
// ... and fp2 with inline products (the G2 bucket sums and reductions of the MSM)
struct fp2i : fp2 {};
LB_HD fp2i f_add(const fp2i& a, const fp2i& b) { return fp2i{fp2_add(a, b)}; }
LB_HD fp2i f_sub(const fp2i& a, const fp2i& b) { return fp2i{fp2_sub(a, b)}; }
LB_HD fp2i f_mul(const fp2i& a, const fp2i& b) {
  const fp t0 = fp_mul_inl(a.c0, b.c0);
  const fp t1 = fp_mul_inl(a.c1, b.c1);
  const fp t2 = fp_mul_inl(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
  return fp2i{fp2{fp_sub(t0, t1), fp_sub(fp_sub(t2, t0), t1)}};
}
LB_HD fp2i f_sqr(const fp2i& a) {
  const fp t0 = fp_mul_inl(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1));
  const fp t1 = fp_mul_inl(a.c0, a.c1);
  return fp2i{fp2{t0, fp_dbl(t1)}};
}
LB_HD fp2i f_dbl(const fp2i& a) { return fp2i{fp2_dbl(a)}; }
LB_HD fp2i f_neg(const fp2i& a) { return fp2i{fp2_neg(a)}; }
LB_HD fp2i f_mul3(const fp2i& a) { return fp2i{fp2_mul3(a)}; }
LB_HD fp2i f_mul8(const fp2i& a) { return fp2i{fp2_mul8(a)}; }
LB_HD bool f_is_zero(const fp2i& a) { return fp2_is_zero(a); }
LB_HD bool f_eq(const fp2i& a, const fp2i& b) { return fp2_eq(a, b); }
LB_HD fp2i f_select(bool c, const fp2i& a, const fp2i& b) { return fp2i{fp2_select(c, a, b)}; }
LB_HD void f_set_zero(fp2i& a) { a = fp2i{fp2_zero()}; }
LB_HD void f_set_one(fp2i& a) { a = fp2i{fp2_one()}; }
LB_HD fp2 f_sub(const fp2& a, const fp2& b) { return fp2_sub(a, b); }
LB_HD fp2 f_mul(const fp2& a, const fp2& b) { return fp2_mul(a, b); }
LB_HD fp2 f_sqr(const fp2& a) { return fp2_sqr(a); }
LB_HD fp2 f_dbl(const fp2& a) { return fp2_dbl(a); }
LB_HD fp2 f_neg(const fp2& a) { return fp2_neg(a); }
LB_HD fp2 f_mul3(const fp2& a) { return fp2_mul3(a); }
LB_HD fp2 f_mul8(const fp2& a) { return fp2_mul8(a); }
LB_HD fp2 f_inv(const fp2& a) { return fp2_inv(a); }
LB_HD bool f_is_zero(const fp2& a) { return fp2_is_zero(a); }
LB_HD bool f_eq(const fp2& a, const fp2& b) { return fp2_eq(a, b); }
LB_HD fp2 f_select(bool c, const fp2& a, const fp2& b) { return fp2_select(c, a, b); }
LB_HD void f_set_zero(fp2& a) { a = fp2_zero(); }
LB_HD void f_set_one(fp2& a) { a = fp2_one(); }
