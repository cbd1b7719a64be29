// Short-Weierstrass (a = 0) group law in Jacobian coordinates, generic over the base
// field (fp for G1: y^2 = x^3 + 4, fp2 for G2: y^2 = x^3 + 4(1+u)).
// Replaces blst's POINTonE1/POINTonE2 arithmetic used by bls.PublicKey.aggregate
// (packages/beacon-node/src/chain/bls/utils.ts:11) and by Pairing.mul_n_aggregate
// (maybeBatch.ts:18-25).  Additions are complete with respect to the cases aggregation
// meets (duplicate keys P == Q, and P == -Q), as SURVEY.md §8 a3 requires.
#pragma once
#include "lb_field.h"

template <class F>
struct jac {
  F x, y, z;  // z == 0 <=> infinity
};
template <class F>
struct aff {
  F x, y;
};

typedef jac<fp> g1j;
typedef jac<fp2> g2j;
typedef aff<fp> g1a;
typedef aff<fp2> g2a;

// the same point over another field type of the same representation (fp <-> fpi)
template <class T, class S>
LB_HD aff<T> aff_as(const aff<S>& a) {
  return aff<T>{T{a.x}, T{a.y}};
}
template <class T, class S>
LB_HD jac<T> jac_as(const jac<S>& a) {
  return jac<T>{T{a.x}, T{a.y}, T{a.z}};
}

template <class F>
LB_HD jac<F> jac_infinity() {
  jac<F> r;
  f_set_one(r.x);
  f_set_one(r.y);
  f_set_zero(r.z);
  return r;
}
template <class F>
LB_HD bool jac_is_inf(const jac<F>& p) {
  return f_is_zero(p.z);
}
template <class F>
LB_HD jac<F> jac_from_aff(const aff<F>& a) {
  jac<F> r;
  r.x = a.x;
  r.y = a.y;
  f_set_one(r.z);
  return r;
}
template <class F>
LB_HD jac<F> jac_neg(const jac<F>& p) {
  return jac<F>{p.x, f_neg(p.y), p.z};
}

// Group operations come in two forms: jac_*_i is force-inlined (the loop bodies of the scalar
// multiplications use it, so the point stays in registers; a by-value jac<> argument of an
// out-of-line call travels through scratch memory), jac_* is the out-of-line wrapper for
// one-off uses.
// dbl-2009-l
template <class F>
LB_HD jac<F> jac_dbl_i(const jac<F>& p) {
  F A = f_sqr(p.x);
  F B = f_sqr(p.y);
  F C = f_sqr(B);
  F D = f_dbl(f_sub(f_sub(f_sqr(f_add(p.x, B)), A), C));
  F E = f_mul3(A);
  F Fv = f_sqr(E);
  jac<F> r;
  r.x = f_sub(Fv, f_dbl(D));
  r.y = f_sub(f_mul(E, f_sub(D, r.x)), f_mul8(C));
  r.z = f_dbl(f_mul(p.y, p.z));
  return r;
}

template <class F>
LB_NI jac<F> jac_dbl(jac<F> p) {
  return jac_dbl_i(p);
}

// add-2007-bl with the exceptional cases handled
// kInl = true keeps the exceptional doubling inline too (a kernel with no out-of-line calls).
template <class F, bool kInl = false>
LB_HD jac<F> jac_add_i(const jac<F>& p, const jac<F>& q) {
  if (jac_is_inf(p)) return q;
  if (jac_is_inf(q)) return p;
  F Z1Z1 = f_sqr(p.z);
  F Z2Z2 = f_sqr(q.z);
  F U1 = f_mul(p.x, Z2Z2);
  F U2 = f_mul(q.x, Z1Z1);
  F S1 = f_mul(f_mul(p.y, q.z), Z2Z2);
  F S2 = f_mul(f_mul(q.y, p.z), Z1Z1);
  F H = f_sub(U2, U1);
  F rr = f_dbl(f_sub(S2, S1));
  if (f_is_zero(H)) {
    if (f_is_zero(rr)) {
      if constexpr (kInl) return jac_dbl_i(p);
      else return jac_dbl(p);
    }
    return jac_infinity<F>();
  }
  F I = f_sqr(f_dbl(H));
  F J = f_mul(H, I);
  F V = f_mul(U1, I);
  jac<F> r;
  r.x = f_sub(f_sub(f_sqr(rr), J), f_dbl(V));
  r.y = f_sub(f_mul(rr, f_sub(V, r.x)), f_dbl(f_mul(S1, J)));
  r.z = f_mul(f_sub(f_sub(f_sqr(f_add(p.z, q.z)), Z1Z1), Z2Z2), H);
  return r;
}

template <class F>
LB_NI jac<F> jac_add(jac<F> p, jac<F> q) {
  return jac_add_i(p, q);
}

// madd-2007-bl: p Jacobian + q affine (q not infinity)
template <class F, bool kInl = false>
LB_HD jac<F> jac_add_aff_i(const jac<F>& p, const aff<F>& q) {
  if (jac_is_inf(p)) return jac_from_aff(q);
  F Z1Z1 = f_sqr(p.z);
  F U2 = f_mul(q.x, Z1Z1);
  F S2 = f_mul(f_mul(q.y, p.z), Z1Z1);
  F H = f_sub(U2, p.x);
  F rr = f_dbl(f_sub(S2, p.y));
  if (f_is_zero(H)) {
    if (f_is_zero(rr)) {
      if constexpr (kInl) return jac_dbl_i(p);
      else return jac_dbl(p);
    }
    return jac_infinity<F>();
  }
  F HH = f_sqr(H);
  F I = f_dbl(f_dbl(HH));
  F J = f_mul(H, I);
  F V = f_mul(p.x, I);
  jac<F> r;
  r.x = f_sub(f_sub(f_sqr(rr), J), f_dbl(V));
  r.y = f_sub(f_mul(rr, f_sub(V, r.x)), f_dbl(f_mul(p.y, J)));
  r.z = f_sub(f_sub(f_sqr(f_add(p.z, H)), Z1Z1), HH);
  return r;
}

template <class F>
LB_NI jac<F> jac_add_aff(jac<F> p, aff<F> q) {
  return jac_add_aff_i(p, q);
}

template <class F>
LB_NI bool jac_eq(jac<F> p, jac<F> q) {
  bool pi = jac_is_inf(p), qi = jac_is_inf(q);
  if (pi || qi) return pi && qi;
  F Z1Z1 = f_sqr(p.z), Z2Z2 = f_sqr(q.z);
  if (!f_eq(f_mul(p.x, Z2Z2), f_mul(q.x, Z1Z1))) return false;
  return f_eq(f_mul(f_mul(p.y, q.z), Z2Z2), f_mul(f_mul(q.y, p.z), Z1Z1));
}

// to affine; returns false for infinity
template <class F>
LB_NI bool jac_to_aff(aff<F>& out, jac<F> p) {
  F zi = f_inv(p.z);
  F zi2 = f_sqr(zi);
  out.x = f_mul(p.x, zi2);
  out.y = f_mul(f_mul(p.y, zi2), zi);
  return !jac_is_inf(p);
}

// Register-only affine conversions for lone-lane stages of the wave kernels (jac_to_aff takes its
// point by value through the stack: a private segment of ~0.7 KB per lane in kernels that run one
// such conversion on one lane).  The only call is the product; the inversion is the inline EEA.
LB_HD void g1_to_aff_inl(g1a& out, const g1j& p) {
  const fp zi = fp_inv_i(p.z), zi2 = fp_sqr(zi);
  out.x = fp_mul(p.x, zi2);
  out.y = fp_mul(fp_mul(p.y, zi2), zi);
}
LB_HD void g2_to_aff_inl(g2a& out, const g2j& p) {
  const fp ni = fp_inv_i(fp_add(fp_sqr(p.z.c0), fp_sqr(p.z.c1)));  // 1/z = conj(z) / N(z)
  const fp2 zi{fp_mul(p.z.c0, ni), fp_neg(fp_mul(p.z.c1, ni))};
  const fp2 zi2 = fp2_sqr(zi);
  out.x = fp2_mul(p.x, zi2);
  out.y = fp2_mul(fp2_mul(p.y, zi2), zi);
}

// [k]P for a 64-bit scalar, P affine (left-to-right double-and-add)
template <class F>
LB_NI jac<F> jac_mul_u64(aff<F> p, uint64_t k) {
  jac<F> acc = jac_infinity<F>();
  for (int i = 63; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((k >> i) & 1ull) acc = jac_add_aff_i(acc, p);
  }
  return acc;
}

// [r]P for a structured blinding scalar.  The 64-bit word w = hi:lo stands for
//   r = lo + hi * lambda  (mod q),  lambda = -x^2 mod q,
// and t1, t2, t3 = P, [lambda]P, P + [lambda]P (affine; free through the endomorphisms, see
// k_pk_blind / k_sig_blind).  Joint double-and-add over the 32 bit pairs: 32 doublings + 32
// mixed additions, against 64 + 64 for a plain 64-bit scalar on a wave (the random bits make
// every wave execute the addition of every step).  The table entry is selected by data, so all
// lanes follow one path.  Distinct words give distinct r (the lattice {(a, b): a + b lambda = 0
// mod q} has no non-zero vector with |a|, |b| < 2^32), so a uniform non-zero word is a uniform
// draw from 2^64 - 1 distinct blinding values, the set size behind blst's 64-bit randomness.
// (jac_mul_glv_i is the inline body: k_pk_blind keeps the table in registers.)
template <class F, bool kInl = false>
LB_HD jac<F> jac_mul_2d_i(const aff<F>& t1, const aff<F>& t2, const aff<F>& t3, uint64_t k0, uint64_t k1, int bits) {
  jac<F> acc = jac_infinity<F>();
  for (int i = bits - 1; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    const uint32_t d = (uint32_t)((k0 >> i) & 1u) | ((uint32_t)((k1 >> i) & 1u) << 1);
    aff<F> t;
    t.x = d == 1u ? t1.x : (d == 2u ? t2.x : t3.x);
    t.y = d == 1u ? t1.y : (d == 2u ? t2.y : t3.y);
    jac<F> s = jac_add_aff_i<F, kInl>(acc, t);
    if (d != 0u) acc = s;
  }
  return acc;
}
template <class F, bool kInl = false>
LB_HD jac<F> jac_mul_glv_i(const aff<F>& t1, const aff<F>& t2, const aff<F>& t3, uint64_t w) {
  return jac_mul_2d_i<F, kInl>(t1, t2, t3, w & 0xffffffffu, w >> 32, 32);
}
template <class F>
LB_NI jac<F> jac_mul_glv(aff<F> t1, aff<F> t2, aff<F> t3, uint64_t w) {
  return jac_mul_glv_i(t1, t2, t3, w);
}

// Fixed-base comb for a key that stays resident (the pubkey table): the same [r]P, r = lo + hi
// lambda, without doublings.  Each 32-bit half is recoded into LB_COMB_J signed radix-16 digits,
//   h = sum_j d_j 16^j,  d_j = nibble_j(h + 0x88888888) - 8 in [-8, 7] (j < 8),  d_8 = the carry,
// and the key's table holds the affine points E[j][d] = [d 16^j]P, d = 1..8 (entry 8 j + d - 1),
// so  [r]P = sum_j sgn(lo_j) E[j][|lo_j|] + sum_j sgn(hi_j) phi(E[j][|hi_j|]),  phi(x, y) = (beta x, y):
// 18 mixed additions and 9 products by beta.  An entry at infinity (a registered point of small
// order, possible only for unvalidated keys) is stored as (0, 0) -- no curve point has y = 0,
// the group order being odd -- and skipped like a zero digit.
#define LB_COMB_J 9
#define LB_COMB_D 8
#define LB_COMB_ENTRIES (LB_COMB_J * LB_COMB_D)
// digit k of the word: k < 9 digit k of lo, else digit k - 9 of hi
LB_HD int comb_digit(uint64_t w, int k) {
  const uint64_t h = (k < LB_COMB_J ? (w & 0xffffffffu) : (w >> 32)) + 0x88888888ull;
  const int j = k < LB_COMB_J ? k : k - LB_COMB_J;
  return j < 8 ? (int)((h >> (4 * j)) & 15u) - 8 : (int)(h >> 32);
}
// the table entry digit k reads (a zero digit reads its position's first entry and discards it)
LB_HD uint32_t comb_entry(uint64_t w, int k) {
  const int d = comb_digit(w, k), a = d < 0 ? -d : d;
  return (uint32_t)(LB_COMB_D * (k < LB_COMB_J ? k : k - LB_COMB_J) + (a ? a - 1 : 0));
}
// E[j][d] = [d 16^j]P (Jacobian), d in [1, 8]
template <class F>
LB_HD jac<F> jac_comb_entry_i(const aff<F>& p, int j, int d) {
  jac<F> acc = jac_infinity<F>();
  for (int b = 3; b >= 0; b--) {
    acc = jac_dbl_i(acc);
    jac<F> s = jac_add_aff_i<F, true>(acc, p);
    if ((d >> b) & 1) acc = s;
  }
  for (int k = 0; k < 4 * j; k++) acc = jac_dbl_i(acc);
  return acc;
}
// ld(e): entry e of the key's table.  The loads of step k + 1 are issued before the addition of
// step k.  The loop stays rolled: one inline addition in the kernel.
template <class F, class Ld>
LB_HD jac<F> jac_mul_comb_i(Ld&& ld, const F& beta, uint64_t w) {
  jac<F> acc = jac_infinity<F>();
  aff<F> nx = ld(comb_entry(w, 0));
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
  for (int k = 0; k < 2 * LB_COMB_J; k++) {
    aff<F> t = nx;
    if (k + 1 < 2 * LB_COMB_J) nx = ld(comb_entry(w, k + 1));
    const int d = comb_digit(w, k);
    const bool skip = d == 0 || f_is_zero(t.y);
    if (k >= LB_COMB_J) t.x = f_mul(t.x, beta);
    t.y = f_select(d < 0, f_neg(t.y), t.y);
    jac<F> s = jac_add_aff_i<F, true>(acc, t);
    if (!skip) acc = s;
  }
  return acc;
}

// [k]P for a 64-bit scalar, P Jacobian (used after aggregation, before the one inversion)
template <class F>
LB_NI jac<F> jac_mul_u64_jac(jac<F> p, uint64_t k) {
  jac<F> acc = jac_infinity<F>();
  for (int i = 63; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((k >> i) & 1ull) acc = jac_add_i(acc, p);
  }
  return acc;
}

// [k]P for a 256-bit scalar (8 little-endian u32 words), P affine.  Synthetic-data helper
// (SecretKey.toPublicKey / SecretKey.sign), not on the verification path.
template <class F>
LB_NI jac<F> jac_mul_u256(aff<F> p, const uint32_t* k) {
  jac<F> acc = jac_infinity<F>();
  for (int i = 255; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((k[i >> 5] >> (i & 31)) & 1u) acc = jac_add_aff_i(acc, p);
  }
  return acc;
}
// [r] P == O for an affine G1 point (r = the BLS12-381 subgroup order): the plain subgroup check of
// G1 points that come from the wire, one-time per point (PublicKey.keyValidate for the resident
// pubkey table; KZG commitments, proofs and setup points, where c-kzg's validate_kzg_g1 rejects
// the same points)
LB_HD bool g1_in_subgroup_r(const aff<fp>& a) {
  const uint32_t rr[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                          0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  return jac_is_inf(jac_mul_u256(a, rr));
}

// [|x|]P for the curve parameter |x| = 0xd201000000010000 (wave-uniform bits)
template <class F, bool kInl = false>
LB_HD jac<F> jac_mul_xabs_i(const jac<F>& p) {
  jac<F> acc = p;  // top bit
  for (int i = 62; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((LB_X_ABS >> i) & 1ull) acc = jac_add_i<F, kInl>(acc, p);
  }
  return acc;
}
template <class F>
LB_NI jac<F> jac_mul_xabs(jac<F> p) {
  return jac_mul_xabs_i(p);
}

// ------------------------------------------------------------------ G2 endomorphism psi
LB_HD g2j g2_psi(const g2j& p) {
  g2j r;
  r.x = fp2_mul(fp2_conj(p.x), fp2_load(LB_PSI_CX));
  r.y = fp2_mul(fp2_conj(p.y), fp2_load(LB_PSI_CY));
  r.z = fp2_conj(p.z);
  return r;
}
LB_HD g2j g2_psi2(const g2j& p) {
  g2j r;
  r.x = fp2_mul_fp(p.x, fp_load(LB_PSI2_CX));
  r.y = fp2_mul_fp(p.y, fp_load(LB_PSI2_CY));
  r.z = p.z;
  return r;
}

// Scott's G2 membership test (the one blst uses): P in G2 <=> psi(P) == [x]P, x < 0.
LB_HD bool g2_in_subgroup(const g2j& p) {
  if (jac_is_inf(p)) return true;
  g2j xp = jac_neg(jac_mul_xabs(p));
  return jac_eq(g2_psi(p), xp);
}

// The same test for an affine point that is not infinity (a decoded signature, z = 1):
// [|x|]P by mixed additions with the loop state in registers, and psi(P) kept affine, so the
// comparison with [x]P = -acc is psi.x Z^2 == X and psi.y Z^3 == -Y.
// Register-lean forms for the two-waves-per-SIMD signature kernels (256 VGPRs).  kInl = true
// inlines the Fp products (fp_mul28 / fp_sqr28): with out-of-line products every value live
// across a call must sit in the ~100 callee-saved VGPRs of the AMDGPU calling convention, which
// the G2 ladder's state overflows.  The statement order is the live-range order: each temporary
// dies as early as the formula allows (dbl-2009-l and madd-2007-bl, reordered; same results as
// jac_dbl_i / jac_add_aff_i).
// (inline products are fenced with scheduling barriers: interleaving the three independent
// products of an Fp2 multiplication would hold three 28-column accumulators at once)
template <bool kInl>
LB_HD fp lean_mul(const fp& a, const fp& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (kInl) {
    __builtin_amdgcn_sched_barrier(0);
    fp r = fp_mul28(a, b);
    __builtin_amdgcn_sched_barrier(0);
    return r;
  }
#endif
  return fp_mul(a, b);
}
template <bool kInl>
LB_HD fp lean_sqr(const fp& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (kInl) {
    __builtin_amdgcn_sched_barrier(0);
    fp r = fp_sqr28(a);
    __builtin_amdgcn_sched_barrier(0);
    return r;
  }
#endif
  return fp_sqr(a);
}
template <bool kInl>
LB_HD fp2 lean2_mul(const fp2& a, const fp2& b) {
  fp t0 = lean_mul<kInl>(a.c0, b.c0);
  fp t1 = lean_mul<kInl>(a.c1, b.c1);
  fp t2 = lean_mul<kInl>(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
  return fp2{fp_sub(t0, t1), fp_sub(fp_sub(t2, t0), t1)};
}
template <bool kInl>
LB_HD fp2 lean2_sqr(const fp2& a) {
  fp t0 = lean_mul<kInl>(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1));
  fp t1 = lean_mul<kInl>(a.c0, a.c1);
  return fp2{t0, fp_dbl(t1)};
}
template <bool kInl>
LB_HD void g2_dbl_lean(g2j& p) {
  p.z = fp2_dbl(lean2_mul<kInl>(p.y, p.z));        // Z3 = 2 Y Z (Z dead)
  fp2 B = lean2_sqr<kInl>(p.y);                    // Y dead from here on
  fp2 C = lean2_sqr<kInl>(B);
  fp2 A = lean2_sqr<kInl>(p.x);
  fp2 D = lean2_sqr<kInl>(fp2_add(p.x, B));        // X, B dead
  D = fp2_dbl(fp2_sub(fp2_sub(D, A), C));
  fp2 E = fp2_mul3(A);                             // A dead
  p.x = fp2_sub(lean2_sqr<kInl>(E), fp2_dbl(D));   // X3
  p.y = fp2_sub(lean2_mul<kInl>(E, fp2_sub(D, p.x)), fp2_mul8(C));
}
// p + q for q affine, p finite (the exceptional cases P == +-Q are handled)
template <bool kInl>
LB_HD void g2_add_aff_lean(g2j& p, const g2a& q) {
  fp2 Z1Z1 = lean2_sqr<kInl>(p.z);
  fp2 H = fp2_sub(lean2_mul<kInl>(q.x, Z1Z1), p.x);    // U2 - X1
  fp2 rr = lean2_mul<kInl>(lean2_mul<kInl>(q.y, p.z), Z1Z1);   // S2
  rr = fp2_dbl(fp2_sub(rr, p.y));
  if (fp2_is_zero(H)) {
    if (fp2_is_zero(rr)) {
      g2_dbl_lean<kInl>(p);
    } else {
      p = jac_infinity<fp2>();
    }
    return;
  }
  fp2 HH = lean2_sqr<kInl>(H);
  p.z = fp2_sub(fp2_sub(lean2_sqr<kInl>(fp2_add(p.z, H)), Z1Z1), HH);  // Z, Z1Z1 dead
  fp2 I = fp2_mul4(HH);                                                  // HH dead
  fp2 J = lean2_mul<kInl>(H, I);                                         // H dead
  fp2 V = lean2_mul<kInl>(p.x, I);                                       // X, I dead
  fp2 YJ = fp2_dbl(lean2_mul<kInl>(p.y, J));                             // Y dead
  p.x = fp2_sub(fp2_sub(lean2_sqr<kInl>(rr), J), fp2_dbl(V));           // J dead
  p.y = fp2_sub(lean2_mul<kInl>(rr, fp2_sub(V, p.x)), YJ);
}

// p + q for Jacobian p, q (add-2007-bl with the exceptional cases, as jac_add_i), register-lean
// statement order for the lone-lane per-root kernels
template <bool kInl>
LB_HD void g2_add_lean(g2j& p, const g2j& q) {
  if (jac_is_inf(q)) return;
  if (jac_is_inf(p)) {
    p = q;
    return;
  }
  const fp2 Z1Z1 = lean2_sqr<kInl>(p.z), Z2Z2 = lean2_sqr<kInl>(q.z);
  const fp2 ZZ = fp2_sub(fp2_sub(lean2_sqr<kInl>(fp2_add(p.z, q.z)), Z1Z1), Z2Z2);  // 2 Z1 Z2
  const fp2 U1 = lean2_mul<kInl>(p.x, Z2Z2);
  const fp2 S1 = lean2_mul<kInl>(lean2_mul<kInl>(p.y, q.z), Z2Z2);
  const fp2 H = fp2_sub(lean2_mul<kInl>(q.x, Z1Z1), U1);
  const fp2 rr = fp2_dbl(fp2_sub(lean2_mul<kInl>(lean2_mul<kInl>(q.y, p.z), Z1Z1), S1));
  if (fp2_is_zero(H)) {
    if (fp2_is_zero(rr)) {
      p = q;
      g2_dbl_lean<kInl>(p);
    } else {
      p = jac_infinity<fp2>();
    }
    return;
  }
  p.z = lean2_mul<kInl>(ZZ, H);
  const fp2 I = lean2_sqr<kInl>(fp2_dbl(H));
  const fp2 J = lean2_mul<kInl>(H, I);
  const fp2 V = lean2_mul<kInl>(U1, I);
  p.x = fp2_sub(fp2_sub(lean2_sqr<kInl>(rr), J), fp2_dbl(V));
  p.y = fp2_sub(lean2_mul<kInl>(rr, fp2_sub(V, p.x)), fp2_dbl(lean2_mul<kInl>(S1, J)));
}

// ---- The psi-ladder in 28-bit limbs end to end (lb_field.h, fp2_28): the same formulas as
// g2_dbl_lean and the mixed addition of k_sig_subgroup, every product fed by the limbs of the
// previous one.  A ladder state is normalised (limbs 0..12 below 2^28) with
//   X <= 30 p,  Y <= 12 p,  Z <= 3 p                                    (LB_L28_VX / VY / VZ)
// per component.  The comments give each value's bound in units of p, a product's as
// 1 + S / 2520 with S the sum of its operand products (for the Fp2 forms the larger of c0's and
// c1's: c0 = a0 b0 + a1 (K - b1) <= a (b + C), the square's (2 a)(a + C)), and <C, S> of a
// subtraction or product is sized to the bounds of what it subtracts: C above its value, 2^S -
// 2^(S-28) above its limbs.  fp2_28_norm stands where a limb bound would otherwise break the
// column condition of the next product, 14 (La Lb + Lc Ld) + 14 x 2^56 + 2^37 < 2^64 (the widest
// here: a first operand of 4 x 2^28 against 2^28 and 2^29), or overflow a word.  The LB_FP28_CHECK host build
// re-derives every bound here on the worst case and aborts where one fails.
#define LB_L28_VX 30.0
#define LB_L28_VY 12.0
#define LB_L28_VZ 3.0
struct g2j28 {
  fp2_28 x, y, z;
};
#if defined(LB_FP28_CHECK)
// the state's tracked bounds are within the invariant; continue from the invariant itself
static inline void fp28_chk_assume(fp28& a, double vb) {
  for (int k = 0; k < 13; k++) LB_CHK_ASSERT(a.ub[k] <= 0x0fffffffu);
  LB_CHK_ASSERT(a.vb <= vb && a.ub[13] <= fp28_chk_top(vb));
  fp28_chk_set(a, vb);
}
static inline void g2j28_chk_assume(g2j28& p) {
  fp28_chk_assume(p.x.c0, LB_L28_VX), fp28_chk_assume(p.x.c1, LB_L28_VX);
  fp28_chk_assume(p.y.c0, LB_L28_VY), fp28_chk_assume(p.y.c1, LB_L28_VY);
  fp28_chk_assume(p.z.c0, LB_L28_VZ), fp28_chk_assume(p.z.c1, LB_L28_VZ);
}
#endif
LB_HD g2j28 g2j28_from_aff(const fp2& x, const fp2& y) {  // below 1.0004 p each
  return g2j28{fp2_28_from_fp2(x), fp2_28_from_fp2(y), fp2_28{fp28_one(), fp28_zero()}};
}
LB_HD g2j28 g2j28_infinity() {
  return g2j28{fp2_28{fp28_one(), fp28_zero()}, fp2_28{fp28_one(), fp28_zero()}, fp2_28{fp28_zero(), fp28_zero()}};
}
// Z == 0 (mod p): the state is redundant, so the test converts down (fp28_is_zero); any value
// below 2^392 is allowed, the state's 3 p is far inside
LB_HD bool g2j28_is_inf(const g2j28& p) { return fp2_28_is_zero(p.z); }
LB_HD g2j g2j28_to_g2j(const g2j28& p) {
  g2j r;
  r.x = fp2_28_to_fp2(p.x);
  r.y = fp2_28_to_fp2(p.y);
  r.z = fp2_28_to_fp2(p.z);
  return r;
}
// dbl-2009-l in the statement order of g2_dbl_lean
LB_HD void g2_dbl_lean28(g2j28& p) {
  LB_CHK(g2j28_chk_assume(p);)
  p.z = fp2_28_norm(fp2_28_muls<2>(fp2_28_mul<13, 28>(p.z, p.y)));  // 2 Y Z: 3 (12 + 13) -> 1.03; 2.06
  const fp2_28 B = fp2_28_sqr<13, 28>(p.y);                         // 24 x 25 -> 1.24
  const fp2_28 C = fp2_28_sqr<2, 28>(B);                            // 2.5 x 3.3 -> 1.004
  const fp2_28 A = fp2_28_sqr<31, 28>(p.x);                         // 60 x 61 -> 2.46
  fp2_28 D = fp2_28_sqr<32, 28>(fp2_28_norm(fp2_28_add(p.x, B)));   // X + B <= 31.3: 62.5 x 63.3 -> 2.57
  D = fp2_28_norm(fp2_28_muls<2>(fp2_28_sub<4, 29>(D, fp2_28_add(A, C))));  // 2 (2.57 + 4) = 13.2; limbs 2^31
  const fp2_28 E = fp2_28_norm(fp2_28_muls<3>(A));                  // 7.4
  p.x = fp2_28_norm(fp2_28_sub<27, 29>(fp2_28_sqr<8, 28>(E), fp2_28_muls<2>(D)));  // 1.09 + 27 = 28.1
  p.y = fp2_28_norm(fp2_28_sub<9, 31>(fp2_28_mul<8, 28>(fp2_28_sub<29, 28>(D, p.x), E),  // 42.2 (7.4 + 8) -> 1.26
                                      fp2_28_muls<8>(C)));                              // + 9 = 10.3
}
// p + q, q affine and read through ld (ld(0) = x, ld(24) = y, 12-word Montgomery form), p finite:
// madd-2007-bl with Z3 = 2 Z1 H as k_sig_subgroup had it.  Returns 0; or 1 for p == q, 2 for
// p == -q, and then p is spent (the ladder replaces it in both cases).  q's coordinates enter as
// the limbs of a 2^8 (up to 256 p) and meet Z1Z1 and Z1^3 (about 1 p) at once.
// Five Fp2 values (140 registers) beside a product's 70 are what 256 registers hold, and the
// formulas want six where q.y and then Y J meet the rest, so Y, and later 2 Y J, wait in the
// caller's parking slot pk (put / get of one fp2_28: LDS in the kernel): the statement order below
// is the live-range order, at most five values across any product.
#if defined(__HIPCC__)
#define LB_HDM __host__ __device__ __forceinline__
#else
#define LB_HDM inline
#endif
struct g2_park28 {  // the host's slot
  fp2_28 v;
  LB_HDM void put(const fp2_28& a) { v = a; }
  LB_HDM fp2_28 get() const { return v; }
};
template <class Ld, class Pk>
LB_HD int g2_madd_lean28(g2j28& p, Ld&& ld, Pk&& pk) {
  LB_CHK(g2j28_chk_assume(p);)
  pk.put(p.y);
  const fp2_28 Z1Z1 = fp2_28_sqr<4, 28>(p.z);                                                      // 6 x 7 -> 1.02
  const fp2_28 H = fp2_28_norm(fp2_28_sub<31, 28>(fp2_28_mul<2, 28>(fp2_28_from_fp2_shift(ld(0)), Z1Z1), p.x));  // 256 x 3.02 -> 1.31; 32.4
  const fp2_28 t = fp2_28_mul<2, 28>(p.z, Z1Z1);                                                   // 1.004; Z1Z1 dead
  const fp2_28 S2 = fp2_28_mul<2, 28>(fp2_28_from_fp2_shift(ld(24)), t);                           // 1.31; t dead
  const fp2_28 rr = fp2_28_norm(fp2_28_muls<2>(fp2_28_sub<13, 28>(S2, pk.get())));                 // 2 (1.31 + 13) = 28.7
  if (fp2_28_is_zero(H)) return fp2_28_is_zero(rr) ? 1 : 2;
  p.z = fp2_28_norm(fp2_28_muls<2>(fp2_28_mul<4, 28>(H, p.z)));         // 32.4 x 7 -> 1.09; 2.2
  const fp2_28 I = fp2_28_muls<4>(fp2_28_sqr<33, 28>(H));               // 64.7 x 65.4 -> 2.68; 10.8, limbs 2^30
  const fp2_28 J = fp2_28_mul<33, 28>(I, H);                            // 10.8 x 65.4 -> 1.28; H dead
  const fp2_28 V = fp2_28_mul<31, 28>(I, p.x);                          // 10.8 x 61 -> 1.27; X, I dead
  pk.put(fp2_28_muls<2>(fp2_28_mul<2, 28>(pk.get(), J)));               // 2 Y J: 12 x 3.3 -> 1.02; 2.04
  p.x = fp2_28_norm(fp2_28_sub<5, 30>(fp2_28_sqr<29, 28>(rr), fp2_28_add(J, fp2_28_muls<2>(V))));  // 57.4 x 57.7 -> 2.32; 7.32; J dead
  const fp2_28 Y3 = fp2_28_mul<29, 28>(fp2_28_sub<8, 28>(V, p.x), rr);                             // 9.3 x 57.7 -> 1.22
  p.y = fp2_28_norm(fp2_28_sub<3, 29>(Y3, pk.get()));                                              // 4.22
  return 0;
}
// Scott's test psi(P) == [x]P for an affine P that is not infinity, P read through ld wherever it
// is used (k_sig_subgroup re-reads it from memory, never holding it across the doublings).  The
// exceptional additions (acc == +-P: points of small order outside G2) reuse the loop's one
// doubling: acc = P, and the next pass's doubling yields acc + P = 2P for the same bit (redo).
// The verdict is that of g2_aff_in_subgroup_i for every input: each decision is a test modulo p.
template <class Ld, class Pk>
LB_HD bool g2_aff_in_subgroup28(Ld&& ld, Pk&& pk) {
  g2j28 acc = g2j28_from_aff(ld(0), ld(24));
  bool redo = false;
#pragma clang loop unroll(disable)
  for (int b = 62; b >= 0;) {
    g2_dbl_lean28(acc);
    if (redo) {
      redo = false;
      b--;
      continue;
    }
    if ((LB_X_ABS >> b) & 1ull) {
      if (g2j28_is_inf(acc)) {
        acc = g2j28_from_aff(ld(0), ld(24));
        b--;
        continue;
      }
      const int e = g2_madd_lean28(acc, ld, pk);
      if (e == 1) {  // acc == P
        acc = g2j28_from_aff(ld(0), ld(24));
        redo = true;
        continue;
      }
      if (e == 2) {  // acc == -P
        acc = g2j28_infinity();
        b--;
        continue;
      }
    }
    b--;
  }
  if (g2j28_is_inf(acc)) return false;  // psi(P) is finite
  const g2j a = g2j28_to_g2j(acc);
  const fp2 z2 = lean2_sqr<true>(a.z);
  if (!fp2_eq(lean2_mul<true>(lean2_mul<true>(fp2_conj(ld(0)), fp2_load(LB_PSI_CX)), z2), a.x)) return false;
  const fp2 py = lean2_mul<true>(fp2_conj(ld(24)), fp2_load(LB_PSI_CY));
  return fp2_eq(lean2_mul<true>(lean2_mul<true>(py, z2), a.z), fp2_neg(a.y));
}

// The loop is kept rolled, and the base point is re-read from memory (`src`, the caller's
// copy) at the five additions instead of being held across the 63 doublings.
LB_HD bool g2_aff_in_subgroup_i(const g2a& a) {
  g2j acc = jac_from_aff(a);
#pragma clang loop unroll(disable)
  for (int i = 62; i >= 0; i--) {
    acc = jac_dbl_i(acc);
    if ((LB_X_ABS >> i) & 1ull) acc = jac_add_aff_i<fp2, true>(acc, a);
  }
  if (jac_is_inf(acc)) return false;  // psi(P) is finite
  fp2 z2 = fp2_sqr(acc.z);
  fp2 px = fp2_mul(fp2_conj(a.x), fp2_load(LB_PSI_CX));
  if (!fp2_eq(fp2_mul(px, z2), acc.x)) return false;
  fp2 py = fp2_mul(fp2_conj(a.y), fp2_load(LB_PSI_CY));
  return fp2_eq(fp2_mul(fp2_mul(py, z2), acc.z), fp2_neg(acc.y));
}

// One share of a test point of the per-batch subgroup check (lb_kernels.h k_subgroup_mix, a lane's;
// DESIGN §5.10): the sum of the bucket sums ld(b), b = first, first + stride, ... < nb, whose bit of
// `bits` (bit b in word b / 32) is set.  The buckets may hold anything on the curve: jac_add_i is complete.
template <class Ld>
LB_HD g2j g2_mix_share(Ld&& ld, const uint32_t* bits, uint32_t first, uint32_t stride, uint32_t nb) {
  g2j v = jac_infinity<fp2>();
  for (uint32_t b = first; b < nb; b += stride)
    if ((bits[b >> 5] >> (b & 31)) & 1u) v = jac_add_i(v, ld(b));
  return v;
}

// h_eff * P via psi (RFC 9380 App. G.3 / Budroni-Pintore)
LB_NI g2j g2_clear_cofactor(g2j p) {
  g2j t1 = jac_neg(jac_mul_xabs(p));  // [x]P
  g2j t2 = g2_psi(p);
  g2j t3 = g2_psi2(jac_dbl(p));
  t3 = jac_add(t3, jac_neg(t2));
  t2 = jac_add(t1, t2);
  t2 = jac_neg(jac_mul_xabs(t2));  // [x](t1 + t2)
  t3 = jac_add(t3, t2);
  t3 = jac_add(t3, jac_neg(t1));
  return jac_add(t3, jac_neg(p));
}

// G1 curve check (affine, y^2 == x^3 + 4)
LB_HD bool g1_aff_on_curve(const g1a& a) {
  return fp_eq(fp_sqr(a.y), fp_add(fp_mul(fp_sqr(a.x), a.x), fp_load(LB_B1)));
}
LB_HD bool g2_aff_on_curve(const g2a& a) {
  return fp2_eq(fp2_sqr(a.y), fp2_add(fp2_mul(fp2_sqr(a.x), a.x), fp2_load(LB_B2)));
}
