// Stand-alone check of the cell calls' host and per-lane pieces (EIP-7594) for a sanitizer build
// (tests/test_kzg_cells_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// deduplication and the combiner (n = 0, 1, 3, a repeated commitment) against the transcript assembled
// by hand; the threaded hashing of five groups against one thread; the phases of k_fr_coset_ntt4096
// against Horner evaluation at the coset points (a random polynomial, zero, X^4095); the cell
// interpolation against the polynomial the cells were evaluated from, and the group sums over 0, 1
// and 65 cells; the quotient lanes through the identity p = Q (X^64 - h^64) + I at a random point and
// on the coset; the status fold of k_kzg_check_cells.  CPU only.
#include <stdio.h>
#include <vector>
#include "kzg_cells_lanes.h"
#include "lb_kzg_transcript.h"

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      failures++;                                                     \
      printf("kzg_cells_check: FAILED line %d: %s\n", __LINE__, #c);  \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static fr rnd_fr() {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = rng32();
  return fr_reduce256(w);
}
static fr digest_fr(const std::vector<uint8_t>& msg) {
  sha_stream s;
  s.update(msg.data(), msg.size());
  return kzg_digest_to_field(s);
}
static void put(std::vector<uint8_t>& v, const void* p, size_t n) {
  v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n);
}
static void put64(std::vector<uint8_t>& v, uint64_t x) {
  uint8_t b[8];
  for (int i = 0; i < 8; i++) b[i] = (uint8_t)(x >> (56 - 8 * i));
  put(v, b, 8);
}
static fr horner(const fr* a, uint32_t n, const fr& x) {
  fr y = fr_zero();
  for (uint32_t k = n; k-- > 0;) y = fr_add(fr_mul(y, x), a[k]);
  return y;
}
static fr pow_u32(const fr& a, uint32_t e) {  // square and multiply over the bits of e alone
  fr acc = fr_one(), sq = a;
  for (; e; e >>= 1, sq = fr_sqr(sq))
    if (e & 1u) acc = fr_mul(acc, sq);
  return acc;
}
// element t of cell i stands at w^(brp7(i) + 128 brp6(t))
static fr coset_point(uint32_t i, uint32_t t) {
  static const fr w = fr_root8192();
  return pow_u32(w, fr_bitrev(i, 7) + 128u * fr_bitrev(t, 6));
}
static fr from_le_words(const uint32_t* w) { return fr_to_mont(fr_from_words(w)); }

// the transcript of one group by hand: `distinct` lists the positions of the distinct commitments
static fr by_hand(uint32_t n, const uint8_t* comms, const std::vector<uint32_t>& distinct, const std::vector<uint32_t>& ci,
                  const uint32_t* idx, const uint8_t* cells, const uint8_t* proofs) {
  std::vector<uint8_t> msg;
  put(msg, "RCKZGCBATCH__V1_", 16);
  put64(msg, 4096);
  put64(msg, 64);
  put64(msg, distinct.size());
  put64(msg, n);
  for (uint32_t d : distinct) put(msg, comms + 48 * d, 48);
  for (uint32_t k = 0; k < n; k++) {
    put64(msg, ci[k]);
    put64(msg, idx[k]);
    put(msg, cells + (size_t)2048 * k, 2048);
    put(msg, proofs + 48 * k, 48);
  }
  return digest_fr(msg);
}

int main() {
  std::vector<fr> tab(LB_FR_CELL_TAB_LEN);
  fr_cell_tables(tab.data());
  {
    const uint32_t rw[8] = LB_FR_ROOT4096_WORDS;
    CHECK(fr_eq(fr_sqr(fr_root8192()), fr_to_mont(fr_from_words(rw))));
    CHECK(fr_eq(fr_mul(tab[LB_FR_CELL_TAB_WINV + 5], tab[LB_FR_CELL_TAB_SCALE + 5]), fr_one()));
    CHECK(fr_eq(tab[LB_FR_CELL_TAB_WINV + fr_cell_h64_index(1)], pow_u32(coset_point(1, 0), 64)));
    CHECK(fr_cell_h64_index(0) == 0);
  }
  // the transcripts
  const uint32_t nk = 8;
  std::vector<uint8_t> comms(nk * 48), proofs(nk * 48), cells((size_t)nk * 2048);
  for (uint8_t& b : comms) b = (uint8_t)rng32();
  for (uint8_t& b : proofs) b = (uint8_t)rng32();
  for (uint8_t& b : cells) b = (uint8_t)rng32();
  std::vector<uint32_t> idx = {0, 127, 64, 5, 5, 6, 99, 1};
  for (uint32_t n : {0u, 1u, 3u}) {
    std::vector<uint32_t> ci(n + 1), first;
    const uint32_t nd = kzg_cell_dedup(n, comms.data(), ci.data(), first);
    CHECK(nd == n && first.size() == n);
    std::vector<uint32_t> want(n);
    for (uint32_t k = 0; k < n; k++) want[k] = k;
    ci.resize(n);
    CHECK(ci == want && first == want);
    const fr r = kzg_cell_batch_r(n, comms.data(), ci.data(), first.data(), nd, idx.data(), cells.data(), proofs.data());
    CHECK(fr_eq(r, by_hand(n, comms.data(), first, ci, idx.data(), cells.data(), proofs.data())));
  }
  {
    // B A B C A with A < B as bytes: first-appearance order, not byte order
    std::vector<uint8_t> c5(5 * 48);
    const int big = memcmp(comms.data(), comms.data() + 48, 48) > 0 ? 0 : 1;
    const uint8_t *B = comms.data() + 48 * big, *A = comms.data() + 48 * (1 - big), *C = comms.data() + 96;
    const uint8_t* seq[5] = {B, A, B, C, A};
    for (int k = 0; k < 5; k++) memcpy(c5.data() + 48 * k, seq[k], 48);
    std::vector<uint32_t> ci(5), first;
    CHECK(kzg_cell_dedup(5, c5.data(), ci.data(), first) == 3);
    CHECK((ci == std::vector<uint32_t>{0, 1, 0, 2, 1}) && (first == std::vector<uint32_t>{0, 1, 3}));
    const fr r = kzg_cell_batch_r(5, c5.data(), ci.data(), first.data(), 3, idx.data(), cells.data(), proofs.data());
    CHECK(fr_eq(r, by_hand(5, c5.data(), first, ci, idx.data(), cells.data(), proofs.data())));
  }
  {
    // five groups of 2, 0, 1, 3, 2 cells; commitments repeat within a group
    const uint32_t off[6] = {0, 2, 2, 3, 6, 8};
    std::vector<uint8_t> c8(nk * 48);
    for (uint32_t k = 0; k < nk; k++) memcpy(c8.data() + 48 * k, comms.data() + 48 * (k % 2), 48);
    std::vector<uint32_t> ci(nk), first, doff(6, 0);
    for (uint32_t g = 0; g < 5; g++)
      doff[g + 1] = doff[g] + kzg_cell_dedup(off[g + 1] - off[g], c8.data() + 48 * off[g], ci.data() + off[g], first);
    CHECK(doff[5] == 2 + 0 + 1 + 2 + 2);
    std::vector<fr> single(5), many(5);
    kzg_cell_batch_rs(5, off, doff.data(), c8.data(), ci.data(), first.data(), idx.data(), cells.data(), proofs.data(), single.data(), 1);
    for (uint32_t g = 0; g < 5; g++) {
      const uint32_t lo = off[g], n = off[g + 1] - lo;
      std::vector<uint32_t> f(first.begin() + doff[g], first.begin() + doff[g + 1]), c(ci.begin() + lo, ci.begin() + lo + n);
      CHECK(fr_eq(single[g], by_hand(n, c8.data() + 48 * lo, f, c, idx.data() + lo, cells.data() + (size_t)2048 * lo, proofs.data() + 48 * lo)));
    }
    for (uint32_t threads : {2u, 5u, 16u}) {
      kzg_cell_batch_rs(5, off, doff.data(), c8.data(), ci.data(), first.data(), idx.data(), cells.data(), proofs.data(), many.data(), threads);
      for (uint32_t g = 0; g < 5; g++) CHECK(fr_eq(many[g], single[g]));
    }
  }
  // the coset transform
  std::vector<fr> poly(4096);
  for (fr& c : poly) c = rnd_fr();
  {
    std::vector<uint32_t> out((size_t)8 * 4096);
    coset_ntt4096_lanes(poly.data(), tab.data(), out.data());
    for (uint32_t k : {0u, 1u, 63u, 64u, 2047u, 4095u}) {
      uint32_t want[8];
      fr_to_be_words(want, horner(poly.data(), 4096, coset_point(64 + k / 64, k % 64)));
      CHECK(memcmp(want, &out[8 * k], 32) == 0);
    }
    std::vector<fr> zero(4096, fr_zero()), top(4096, fr_zero());
    coset_ntt4096_lanes(zero.data(), tab.data(), out.data());
    bool all_zero = true;
    for (uint32_t w : out) all_zero &= w == 0;
    CHECK(all_zero);
    top[4095] = fr_one();
    coset_ntt4096_lanes(top.data(), tab.data(), out.data());
    for (uint32_t k : {0u, 1u, 100u, 4095u}) {
      uint32_t want[8];
      fr_to_be_words(want, pow_u32(coset_point(64 + k / 64, k % 64), 4095));
      CHECK(memcmp(want, &out[8 * k], 32) == 0);
    }
  }
  // interpolation and group sums: 66 cells evaluated from known polynomials of degree < 64
  {
    const uint32_t nc = 66, off[4] = {0, 0, 1, 66};
    std::vector<uint32_t> ix(nc);
    std::vector<fr> coeffs((size_t)nc * 64), vals((size_t)nc * 64), wt(nc);
    for (uint32_t c = 0; c < nc; c++) {
      ix[c] = c < 4 ? (c == 0 ? 0u : c == 1 ? 1u : c == 2 ? 64u : 127u) : rng32() % 128;
      wt[c] = c < 5 ? fr_one() : rnd_fr();
      for (uint32_t j = 0; j < 64; j++) coeffs[(size_t)c * 64 + j] = (c == 4 && j > 0) ? fr_zero() : rnd_fr();  // cell 4: a constant
      for (uint32_t t = 0; t < 64; t++) vals[(size_t)c * 64 + t] = horner(&coeffs[(size_t)c * 64], 64, coset_point(ix[c], t));
    }
    for (uint32_t t = 1; t < 64; t++) CHECK(fr_eq(vals[4 * 64 + t], vals[4 * 64]));
    cell_interp_lanes(nc, vals.data(), ix.data(), wt.data(), tab.data());
    for (size_t i = 0; i < (size_t)nc * 64; i++) CHECK(fr_eq(vals[i], fr_mul(wt[i / 64], coeffs[i])));
    std::vector<uint32_t> sums((size_t)3 * 64 * 8);
    cell_sum_lanes(3, off, nc, vals.data(), sums.data());
    for (uint32_t g = 0; g < 3; g++)
      for (uint32_t j = 0; j < 64; j++) {
        fr acc = fr_zero();
        for (uint32_t c = off[g]; c < off[g + 1]; c++) acc = fr_add(acc, fr_mul(wt[c], coeffs[(size_t)c * 64 + j]));
        CHECK(fr_eq(fr_neg(acc), from_le_words(&sums[((size_t)g * 64 + j) * 8])));
      }
  }
  // the quotient lanes
  for (uint32_t cell : {0u, 127u}) {
    const fr c64 = pow_u32(coset_point(cell, 0), 64);
    for (int low = 0; low < 2; low++) {
      std::vector<fr> a(poly);
      if (low)
        for (uint32_t j = 64; j < 4096; j++) a[j] = fr_zero();
      std::vector<uint32_t> q_le((size_t)8 * 4096, 0xAAAAAAAAu);
      cell_quotient_lanes(a.data(), cell, tab.data(), q_le.data());
      std::vector<fr> q(4096), rem(64);
      for (uint32_t j = 0; j < 4096; j++) q[j] = from_le_words(&q_le[8 * j]);
      for (uint32_t j = 4032; j < 4096; j++) CHECK(fr_is_zero(q[j]));
      if (low)
        for (uint32_t j = 0; j < 4096; j++) CHECK(fr_is_zero(q[j]));
      for (uint32_t j = 0; j < 64; j++) rem[j] = fr_add(a[j], fr_mul(c64, q[j]));
      const fr x = rnd_fr();
      CHECK(fr_eq(horner(a.data(), 4096, x),
                  fr_add(fr_mul(horner(q.data(), 4096, x), fr_sub(pow_u32(x, 64), c64)), horner(rem.data(), 64, x))));
      for (uint32_t t : {0u, 1u, 63u}) {
        const fr h = coset_point(cell, t);
        CHECK(fr_eq(horner(a.data(), 4096, h), horner(rem.data(), 64, h)));
      }
    }
  }
  // the status fold: groups of 0, 1 and 3 cells, the last with two distinct commitments
  {
    const uint32_t off[4] = {0, 0, 1, 4}, doff[4] = {0, 0, 1, 3};
    auto fold = [&](uint32_t g, const int32_t* d, const int32_t* c, const int32_t* p) {
      return kzg_cell_group_status(d, doff[g], doff[g + 1], c, p, off[g], off[g + 1]);
    };
    int32_t d[3] = {0, 0, 0}, c[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0};
    for (uint32_t g = 0; g < 3; g++) CHECK(fold(g, d, c, p) == LB_OK);
    p[3] = LB_POINT_NOT_IN_GROUP;
    CHECK(fold(2, d, c, p) == LB_POINT_NOT_IN_GROUP && fold(1, d, c, p) == LB_OK);
    p[1] = 1;
    CHECK(fold(2, d, c, p) == 1);
    c[3] = 7;
    CHECK(fold(2, d, c, p) == LB_BAD_SCALAR);
    d[2] = LB_POINT_NOT_IN_GROUP;
    CHECK(fold(2, d, c, p) == LB_POINT_NOT_IN_GROUP);
    d[1] = 1;
    CHECK(fold(2, d, c, p) == 1 && fold(1, d, c, p) == LB_OK && fold(0, d, c, p) == LB_OK);
    c[0] = LB_BAD_SCALAR;
    CHECK(fold(1, d, c, p) == LB_BAD_SCALAR);
    d[0] = LB_POINT_NOT_IN_GROUP;
    CHECK(fold(1, d, c, p) == LB_POINT_NOT_IN_GROUP);
  }
  printf("kzg_cells_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
