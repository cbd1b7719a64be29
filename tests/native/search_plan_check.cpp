// Stand-alone check of the invalid-set search's planner and interpreter (lodestar_amd/csrc/
// lb_search_plan.h through tests/harness/search_model.h) for a sanitizer build
// (tests/test_search_plan_cpu.py builds it with -fsanitize=address,undefined and runs it): 384 random
// layouts (n up to 5 000, every combination of spec_on, r1_plain, rs and search_small_max 0 / 64 /
// 32 768) whose search must name exactly the failing sets with no table invariant violated; the
// directed layouts (a root above the weighted part cap, nu at the tree's edges, every set failing at
// n = 300, a round split by the instance budget); the three lying models; the blocks helper and the
// map to jobs at their edges.  The planner is index arithmetic over vectors: out-of-range reads and
// overflowing shifts are what this build catches.  CPU only.
#include <stdio.h>

#include "search_model.h"

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      failures++;                                                      \
      printf("search_plan_check: FAILED line %d: %s\n", __LINE__, #c); \
    }                                                                  \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

// n sets over nu roots, every root used, roots numbered by first occurrence
static std::vector<uint32_t> layout(uint32_t n, uint32_t nu) {
  std::vector<uint32_t> r(n);
  for (uint32_t i = 0; i < n; i++) r[i] = i < nu ? i : rng32() % nu;
  for (uint32_t i = n - 1; i > 0; i--) std::swap(r[i], r[rng32() % (i + 1)]);
  std::vector<uint32_t> rank(nu, UINT32_MAX);
  uint32_t next = 0;
  for (uint32_t& u : r) {
    if (rank[u] == UINT32_MAX) rank[u] = next++;
    u = rank[u];
  }
  return r;
}

// runs one search; true iff no invariant was violated and the sets found are `want` exactly
static bool search_finds(const std::vector<uint32_t>& roots, uint32_t nu, const std::vector<uint8_t>& bad, uint32_t flags,
                         uint32_t small_max, int lie, bool want_all, search_result* out = nullptr) {
  search_case c;
  search_layout(c.x, roots, nu);
  c.x.rs = (flags & 4u) != 0;
  c.bad = bad;
  c.spec_on = (flags & 1u) != 0;
  c.r1_plain = (flags & 2u) != 0;
  c.small_max = small_max;
  c.lie = lie;
  search_result r;
  search_run(c, r);
  for (const std::string& s : r.violations) printf("search_plan_check: %s\n", s.c_str());
  std::vector<uint32_t> hits(c.x.n, 0);
  for (uint32_t p : r.bad_pos) hits[c.x.members[p]]++;
  bool ok = r.violations.empty();
  for (uint32_t i = 0; i < c.x.n; i++) ok &= hits[i] == ((want_all || bad[i]) ? 1u : 0u);
  if (out) *out = r;
  return ok;
}

int main() {
  const uint32_t small[3] = {0, 64, 32768};
  for (uint32_t it = 0; it < 384; it++) {
    const uint32_t n = 1 + rng32() % ((it & 3u) ? 5000u : 150u), nu = 1 + rng32() % ((it % 5u) ? n : std::min(n, 6u));
    const std::vector<uint32_t> roots = layout(n, nu);
    std::vector<uint8_t> bad(n, 0);
    const uint32_t k = 1 + ((it % 16u) ? rng32() % 6u : rng32() % n);  // the search runs after a failing root check
    for (uint32_t j = 0; j < k; j++) bad[rng32() % n] = 1;
    search_result r;
    CHECK(search_finds(roots, nu, bad, it & 7u, small[(it >> 3) % 3u], LIE_NONE, false, &r));
    CHECK(r.rounds <= kMaxRounds);
  }
  {  // a root above the weighted part cap: 2 200 sets over 2 roots
    const std::vector<uint32_t> roots = layout(2200, 2);
    std::vector<uint8_t> bad(2200, 0);
    bad[3] = bad[1099] = bad[2150] = 1;
    for (uint32_t flags = 0; flags < 8; flags++) CHECK(search_finds(roots, 2, bad, flags, small[flags % 3u], LIE_NONE, false));
  }
  for (uint32_t nu : {1u, 2u, 64u, 65u, 4096u, 4097u})
    for (uint32_t n : {nu, nu + 1, std::min(5000u, 2 * nu + 37)}) {
      const std::vector<uint32_t> roots = layout(n, nu);
      std::vector<uint8_t> bad(n, 0);
      bad[0] = bad[n - 1] = bad[rng32() % n] = 1;
      for (uint32_t flags = 0; flags < 8; flags++) CHECK(search_finds(roots, nu, bad, flags, small[flags % 3u], LIE_NONE, false));
    }
  for (uint32_t nu : {1u, 7u, 300u})  // every set failing
    for (uint32_t flags = 0; flags < 8; flags++)
      CHECK(search_finds(layout(300, nu), nu, std::vector<uint8_t>(300, 1), flags, small[flags % 3u], LIE_NONE, false));
  {  // the instance budget splits a round
    std::vector<uint32_t> roots(5000);
    for (uint32_t i = 0; i < 5000; i++) roots[i] = i / 2;
    search_result r;
    CHECK(search_finds(roots, 2500, std::vector<uint8_t>(5000, 1), 1u, 32768, LIE_NONE, false, &r));
    bool split = false;
    for (size_t i = 5; i < r.trace.size(); i += 5) split |= r.trace[i] == r.trace[i - 5];
    CHECK(split);
  }
  {  // the lying models fail closed
    const std::vector<uint32_t> roots = layout(500, 40);
    std::vector<uint8_t> bad(500, 0);
    bad[17] = bad[300] = 1;
    search_result r;
    CHECK(search_finds(roots, 40, bad, 1u, 32768, LIE_PASS, true, &r));
    CHECK(r.rounds == 1);
    CHECK(search_finds(roots, 40, bad, 1u, 32768, LIE_TOUT, false, &r));
    CHECK(r.rounds <= kMaxRounds);
    CHECK(search_finds(roots, 40, bad, 1u, 32768, LIE_STALL, true, &r));
    CHECK(r.rounds == kMaxRounds + 1);
  }
  {  // blocks of at most 64: empty ranges, 64, 65, a prefix array that does not start at 0
    const std::vector<uint32_t> pre{9, 9, 10, 74, 139, 139, 339};
    std::vector<uint32_t> blo, bhi, bo;
    blocks64(pre.data(), (uint32_t)pre.size() - 1, blo, bhi, bo);
    CHECK(bo == (std::vector<uint32_t>{0, 0, 1, 2, 4, 4, 8}));
    CHECK(blo == (std::vector<uint32_t>{9, 10, 74, 138, 139, 203, 267, 331}));
    CHECK(bhi == (std::vector<uint32_t>{10, 74, 138, 139, 203, 267, 331, 339}));
    blocks64(pre.data(), 0, blo, bhi, bo);
    CHECK(blo.empty() && bhi.empty() && bo == std::vector<uint32_t>{0});
  }
  {  // failing positions -> jobs: only a job that was 1 changes; empty jobs, the last set
    search_ctx x;
    x.n = 6;
    x.members = {5, 0, 3, 1, 4, 2};
    const std::vector<uint32_t> job_off{0, 2, 2, 3, 6};
    int32_t out[4] = {1, 1, -6, 1};
    search_jobs(x, {0, 2}, job_off, 4, out);  // sets 5 and 3
    CHECK(out[0] == 1 && out[1] == 1 && out[2] == -6 && out[3] == 0);
    search_jobs(x, {1, 5}, job_off, 4, out);  // sets 0 and 2 (job 2 was rejected before: stays)
    CHECK(out[0] == 0 && out[1] == 1 && out[2] == -6 && out[3] == 0);
  }
  printf("search_plan_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
