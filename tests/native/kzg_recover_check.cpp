// Stand-alone check of the recovery pieces (lb_recover.h through tests/harness/kzg_recover_lanes.h,
// and lb_kzg_host.h's argument check) for a sanitizer build (tests/test_kzg_recover_cpu.py builds it
// with -fsanitize=address,undefined and runs it).  For the polynomials dense, degree 70, X^4095,
// constant and zero and the index sets 0..63, 64..127, evens, odds, a random 64, a random 65, all but
// cell 0, all but cell 127 and all 128: the given cells' interpolation polynomials are written down
// from the identity P_r(y_i) by Horner (no transform shared with the code under test), the decode
// must return the coefficients with every upper half zero, and Zev / 1 / Zc must equal the product
// over the missing cells taken directly (missing sets of 0, 1, 63 and 64 cells among them).  A changed
// value among 65 cells must raise the flag; among 64 it must not, and the recovered polynomial then
// takes the changed value.  The slot map, the rank, the write-back index, the argument check and the
// blob's elements from its coefficients (against Horner at a few roots) are checked too.  CPU only.
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "kzg_recover_lanes.h"
#include "lb_kzg_host.h"

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      failures++;                                                       \
      printf("kzg_recover_check: FAILED line %d: %s\n", __LINE__, #c);  \
    }                                                                   \
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
static fr pow_u32(const fr& a, uint32_t e) {
  fr acc = fr_one(), sq = a;
  for (; e; e >>= 1, sq = fr_sqr(sq))
    if (e & 1u) acc = fr_mul(acc, sq);
  return acc;
}
static uint32_t brp(uint32_t i, int bits) {
  uint32_t r = 0;
  for (int b = 0; b < bits; b++)
    if (i & (1u << b)) r |= 1u << (bits - 1 - b);
  return r;
}
static fr w128() { return pow_u32(fr_root8192(), 64); }

static std::vector<fr> fk, tab;

// cell i's interpolation polynomial by the identity: coefficient r is P_r(y_i), P_r[k] = a[64 k + r]
static void interp_of(const std::vector<fr>& a, uint32_t cell, fr* out) {
  const fr y = pow_u32(w128(), brp(cell, 7));
  for (uint32_t r = 0; r < 64; r++) {
    fr acc = fr_zero();
    for (int k = 63; k >= 0; k--) acc = fr_add(fr_mul(acc, y), a[64 * k + r]);
    out[r] = acc;
  }
}
static std::vector<uint32_t> random_set(uint32_t n) {
  std::vector<uint32_t> all(128);
  for (uint32_t i = 0; i < 128; i++) all[i] = i;
  for (uint32_t i = 127; i > 0; i--) std::swap(all[i], all[rng32() % (i + 1)]);
  all.resize(n);
  std::sort(all.begin(), all.end());
  return all;
}

struct decoded {
  bool planned;
  std::vector<fr> coef;
  bool flag, upper_nonzero;
};
// one index set's mask and vanishing values, computed once for all polynomials
struct planned_set {
  std::vector<uint32_t> idx;
  bool ok;
  uint32_t mask[LB_RC_MASK_WORDS];
  fr zev[128], zcinv[128];
  explicit planned_set(const std::vector<uint32_t>& i) : idx(i), mask{0, 0, 0, 0} {
    const uint32_t off[2] = {0, (uint32_t)idx.size()};
    ok = kzg_recover_plan(1, off, idx.data(), mask);
    if (ok) rc_zero_lanes(mask, fk.data(), tab.data(), zev, zcinv);
  }
};
// the call's decode for one blob from interpolated cells
static decoded decode(const planned_set& ps, const std::vector<fr>& cells) {
  decoded d{ps.ok, std::vector<fr>(4096), false, false};
  if (!ps.ok) return d;
  fr upper[64];
  for (uint32_t r = 0; r < 64; r++) {
    d.flag |= rc_col_lanes(cells.data(), (uint32_t)ps.idx.size(), 0, ps.mask, ps.zev, ps.zcinv, fk.data(), tab.data(), r,
                           d.coef.data(), upper);
    for (const fr& u : upper) d.upper_nonzero |= !fr_is_zero(u);
  }
  return d;
}
// all 128 interpolated cells of a polynomial, and a choice of them
static std::vector<fr> interp_all(const std::vector<fr>& a) {
  std::vector<fr> all(128 * 64);
  for (uint32_t i = 0; i < 128; i++) interp_of(a, i, &all[64 * i]);
  return all;
}
static std::vector<fr> chosen(const std::vector<fr>& all, const std::vector<uint32_t>& idx) {
  std::vector<fr> cells(idx.size() * 64);
  for (size_t k = 0; k < idx.size(); k++) std::copy(&all[64 * idx[k]], &all[64 * idx[k]] + 64, &cells[64 * k]);
  return cells;
}
static bool same(const std::vector<fr>& a, const std::vector<fr>& b) {
  for (size_t i = 0; i < a.size(); i++)
    if (!fr_eq(a[i], b[i])) return false;
  return a.size() == b.size();
}

static void check_zero(const std::vector<uint32_t>& idx) {
  uint32_t mask[4] = {0, 0, 0, 0};
  for (uint32_t i : idx) mask[i >> 5] |= 1u << (i & 31);
  fr zev[128], zcinv[128];
  rc_zero_lanes(mask, fk.data(), tab.data(), zev, zcinv);
  const fr s = fr_root8192();
  bool ok = true;
  for (uint32_t m = 0; m < 128; m++) {
    const fr x = pow_u32(w128(), m);
    fr a = fr_one(), c = fr_one();
    for (uint32_t i = 0; i < 128; i++) {
      if (std::binary_search(idx.begin(), idx.end(), i)) continue;
      const fr y = pow_u32(w128(), brp(i, 7));
      a = fr_mul(a, fr_sub(x, y));
      c = fr_mul(c, fr_sub(fr_mul(s, x), y));
    }
    ok &= fr_eq(zev[m], a) && fr_eq(fr_mul(zcinv[m], c), fr_one());
  }
  CHECK(ok);
}

static void check_maps() {
  bool ok = true;
  for (uint32_t i = 0; i < 128; i++) ok &= rc_point(i) == brp(i, 7) && rc_slot(i) == i;
  CHECK(ok);
  const std::vector<uint32_t> idx = random_set(65);
  uint32_t mask[4] = {0, 0, 0, 0};
  for (uint32_t i : idx) mask[i >> 5] |= 1u << (i & 31);
  ok = true;
  for (uint32_t k = 0; k < idx.size(); k++) ok &= rc_rank(mask, idx[k]) == k && rc_present(mask, idx[k]);
  CHECK(ok);
  std::vector<int> seen(4096, 0);
  for (uint32_t k = 0; k < 64; k++)
    for (uint32_t r = 0; r < 64; r++) seen[rc_coef_index(k, r)]++;
  CHECK(std::count(seen.begin(), seen.end(), 1) == 4096);
  CHECK(rc_coef_index(1, 0) == 64 && rc_coef_index(0, 63) == 63);
}

static void check_plan() {
  std::vector<uint32_t> idx(129), mask(8);
  for (uint32_t i = 0; i < 129; i++) idx[i] = i;
  const uint32_t o63[2] = {0, 63}, o64[2] = {0, 64}, o128[2] = {0, 128}, o129[2] = {0, 129}, o1[2] = {1, 65};
  auto plan = [&](const uint32_t* off, const uint32_t* ix) {
    std::fill(mask.begin(), mask.end(), 0u);
    return kzg_recover_plan(1, off, ix, mask.data());
  };
  CHECK(!plan(o63, idx.data()));
  CHECK(plan(o64, idx.data()) && mask[0] == 0xffffffffu && mask[1] == 0xffffffffu && mask[2] == 0 && mask[3] == 0);
  CHECK(plan(o128, idx.data()) && mask[3] == 0xffffffffu);
  CHECK(!plan(o129, idx.data()));
  CHECK(!plan(o1, idx.data()));
  CHECK(!plan(o64, idx.data() + 65));  // 65 .. 128: an index past the last cell
  std::vector<uint32_t> dup(idx.begin(), idx.begin() + 64), desc(dup);
  dup[63] = 62;
  std::swap(desc[10], desc[11]);
  CHECK(!plan(o64, dup.data()));
  CHECK(!plan(o64, desc.data()));
  const uint32_t two[3] = {0, 64, 127};
  std::fill(mask.begin(), mask.end(), 0u);
  CHECK(!kzg_recover_plan(2, two, idx.data(), mask.data()));  // the second blob is short
  const uint32_t dec[3] = {0, 64, 0};
  CHECK(!kzg_recover_plan(2, dec, idx.data(), mask.data()));
}

static void check_blob(const std::vector<fr>& a) {
  std::vector<fr> v(4096);
  rc_blob_lanes(a.data(), tab.data(), 1024, v.data());
  const fr w4096 = fr_sqr(fr_root8192());
  const uint32_t ks[5] = {0, 1, 2, 1000, 4095};
  for (uint32_t k : ks) {
    const fr x = pow_u32(w4096, brp(k, 12));
    fr acc = fr_zero();
    for (int j = 4095; j >= 0; j--) acc = fr_add(fr_mul(acc, x), a[j]);
    CHECK(fr_eq(v[k], acc));
  }
}

int main() {
  fk.resize(LB_FK_TAB_LEN);
  tab.resize(LB_FR_CELL_TAB_LEN);
  fk_tables(fk.data());
  fr_cell_tables(tab.data());
  check_maps();
  check_plan();

  std::vector<std::vector<uint32_t>> sets(9);
  for (uint32_t i = 0; i < 64; i++) {
    sets[0].push_back(i);
    sets[1].push_back(64 + i);
    sets[2].push_back(2 * i);
    sets[3].push_back(2 * i + 1);
  }
  sets[4] = random_set(64);
  sets[5] = random_set(65);
  for (uint32_t i = 0; i < 128; i++) {
    if (i != 0) sets[6].push_back(i);
    if (i != 127) sets[7].push_back(i);
    sets[8].push_back(i);
  }
  for (const auto& s : sets) check_zero(s);  // missing sets of 64, 63, 1 and 0 cells

  std::vector<std::vector<fr>> polys(5, std::vector<fr>(4096, fr_zero())), interp;
  for (auto& x : polys[0]) x = rnd_fr();
  for (uint32_t j = 0; j <= 70; j++) polys[1][j] = rnd_fr();
  polys[2][4095] = fr_one();
  polys[3][0] = rnd_fr();
  for (const auto& a : polys) {
    interp.push_back(interp_all(a));
    check_blob(a);
  }
  std::vector<planned_set> plans(sets.begin(), sets.end());
  for (const planned_set& ps : plans)
    for (size_t k = 0; k < polys.size(); k++) {
      const decoded d = decode(ps, chosen(interp[k], ps.idx));
      CHECK(d.planned && !d.flag && !d.upper_nonzero && same(d.coef, polys[k]));
    }

  // one value changed: among 65 cells the flag, among 64 another polynomial that takes the value
  std::vector<fr> cells = chosen(interp[0], sets[5]);
  cells[64 * 3 + 17] = fr_add(cells[64 * 3 + 17], fr_one());
  decoded d = decode(plans[5], cells);
  CHECK(d.planned && d.flag && d.upper_nonzero);
  cells = chosen(interp[0], sets[4]);
  cells[64 * 3 + 17] = fr_add(cells[64 * 3 + 17], fr_one());
  d = decode(plans[4], cells);
  CHECK(d.planned && !d.flag && !d.upper_nonzero && !same(d.coef, polys[0]));
  CHECK(same(chosen(interp_all(d.coef), sets[4]), cells));

  printf("kzg_recover_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
