// CPU harness of the resident pubkey table's fixed-base comb (lb_curve.h jac_comb_entry_i /
// jac_mul_comb_i, the code k_comb_fill and k_pk_blind_comb run), compiled as plain C++ for
// tests/test_pk_comb_cpu.py.  Test infrastructure only; the product path is the HIP build.
#include <string.h>
#include "lb_serial.h"
#if defined(LB_COUNT_OPS)
unsigned long long lb_count_mul = 0;  // tools/count_ops.py: Fp multiplications of one comb(P, w)
#endif

static fp rd(const uint8_t* b) { fp x; fp_plain_from_be48(x, b, 0xff); return fp_to_mont(x); }
static void wr(uint8_t* b, const fp& a) { fp_plain_to_be48(b, fp_from_mont(a)); }
static g1a rdg1(const uint8_t* b) { return g1a{rd(b), rd(b + 48)}; }
static int wrg1(uint8_t* b, const g1j& p) { g1a a; bool ok = jac_to_aff(a, p); wr(b, a.x); wr(b + 48, a.y); return ok; }

extern "C" {
int c_comb_entries(void) { return LB_COMB_ENTRIES; }
int c_comb_entry_bytes(void) { return (int)sizeof(g1a); }
// the 18 signed digits of a word and the entry each one reads
void c_comb_digits(uint64_t w, int32_t* digits18, uint32_t* entries18) {
  for (int k = 0; k < 2 * LB_COMB_J; k++) {
    digits18[k] = comb_digit(w, k);
    entries18[k] = comb_entry(w, k);
  }
}
// one key's table as the device stores it: LB_COMB_ENTRIES records of 96 B, Montgomery limbs,
// entry 8 j + d - 1 = [d 16^j]P affine; an entry at infinity is all zero
void c_comb_build(const uint8_t* p96, uint8_t* table) {
  const g1a p = rdg1(p96);
  for (int j = 0; j < LB_COMB_J; j++)
    for (int d = 1; d <= LB_COMB_D; d++) {
      const g1j e = jac_comb_entry_i<fp>(p, j, d);
      g1a a{fp_zero(), fp_zero()};
      if (!jac_is_inf(e)) jac_to_aff(a, e);
      memcpy(table + sizeof(g1a) * (LB_COMB_D * j + d - 1), &a, sizeof(g1a));
    }
}
// comb(P, w) from the table -> affine, 96 bytes big-endian; returns 0 for infinity
int c_comb_mul(const uint8_t* table, uint64_t w, uint8_t* out96) {
  const g1j r = jac_mul_comb_i<fp>(
      [&](uint32_t e) { g1a a; memcpy(&a, table + sizeof(g1a) * e, sizeof(g1a)); return a; }, fp_load(LB_GLV_BETA), w);
  return wrg1(out96, r);
}
#if defined(LB_COUNT_OPS)
unsigned long long cnt_g1_comb(const uint8_t* table, uint64_t w) {
  lb_count_mul = 0;
  jac_mul_comb_i<fp>([&](uint32_t e) { g1a a; memcpy(&a, table + sizeof(g1a) * e, sizeof(g1a)); return a; },
                     fp_load(LB_GLV_BETA), w);
  return lb_count_mul;
}
#endif
// the reference: the GLV ladder k_pk_blind runs
int c_glv_mul(const uint8_t* p96, uint64_t w, uint8_t* out96) {
  const g1a p = rdg1(p96);
  const g1a t2{fp_mul(p.x, fp_load(LB_GLV_BETA)), p.y};
  const g1a t3{fp_mul(p.x, fp_load(LB_GLV_BETA2)), fp_neg(p.y)};
  return wrg1(out96, jac_mul_glv(p, t2, t3, w));
}
}
