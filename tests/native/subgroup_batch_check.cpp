// Host check of the per-batch signature subgroup test: the selection
// (lb_pipeline_plan.h pipe_plan_subgroup_batch) over its whole grid, and the mixing of bucket sums
// (lb_curve.h g2_mix_share, the code k_subgroup_mix runs per lane, and the 64 lanes' sum) with
// Scott's test on the mixed points, over a small bucket array filled from
// tests/golden/subgroup28_points.txt (argv[1]): points of G2, curve points of large cofactor
// order, points of order 13 and 23, sums of both.  Every bucket is formed by the additions of the
// MSM path (jac_add_aff_i into a chunk sum, jac_add_i of chunk sums), so P + P and P + (-P) of
// points outside G2 go through them here.  Because the torsion part of a mixed point is the sum of
// the picked dirty buckets' torsion parts, the program knows for every single test whether it must
// pass, not only for the batch.  tests/test_subgroup_batch_cpu.py builds it with g++, plain and
// with -fsanitize=address,undefined, and reads the lines it prints.  No GPU.
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "lb_curve.h"
#include "lb_pipeline_plan.h"

static int g_bad = 0, g_checks = 0;
#define EXPECT(c)                                           \
  do {                                                      \
    g_checks++;                                             \
    if (!(c)) {                                             \
      g_bad++;                                              \
      if (g_bad < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                       \
  } while (0)

constexpr uint32_t kBuckets = 16, kTests = 64, kLanes = 4;  // lanes: shares of a test point, as the wave's 64

struct pt {
  std::string kind;
  int in_group;
  g2a a;
};
static fp parse_fp(const char* hex) {  // 96 hex digits, plain integer -> Montgomery words
  fp a = fp_zero();
  for (int i = 0; i < 96; i++) {
    const char c = hex[95 - i];
    const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    a.v[i / 8] |= d << (4 * (i % 8));
  }
  return fp_to_mont(a);
}
static std::vector<pt> load_points(const char* path) {
  std::vector<pt> out;
  FILE* f = fopen(path, "r");
  if (!f) return out;
  char kind[32], h[4][128];
  int e;
  while (fscanf(f, "%31s %d %127s %127s %127s %127s", kind, &e, h[0], h[1], h[2], h[3]) == 6) {
    pt p;
    p.kind = kind, p.in_group = e;
    p.a.x = fp2{parse_fp(h[0]), parse_fp(h[1])};
    p.a.y = fp2{parse_fp(h[2]), parse_fp(h[3])};
    out.push_back(p);
  }
  fclose(f);
  return out;
}
static std::vector<g2a> of_kind(const std::vector<pt>& pts, const char* kind) {
  std::vector<g2a> out;
  for (const pt& p : pts)
    if (p.kind == kind) out.push_back(p.a);
  return out;
}
static g2a neg(const g2a& a) { return g2a{a.x, fp2_neg(a.y)}; }

// a bucket as the MSM forms it: chunk sums of its members by mixed additions, then the chunk sums added
static g2j bucket_of(const std::vector<g2a>& members) {
  g2j sum = jac_infinity<fp2>();
  for (size_t c = 0; c < members.size(); c += 2) {
    g2j acc = jac_infinity<fp2>();
    for (size_t k = c; k < members.size() && k < c + 2; k++) acc = jac_add_aff_i<fp2, true>(acc, members[k]);
    sum = jac_add_i<fp2, true>(sum, acc);
  }
  return sum;
}

// Scott's test on a mixed point, infinity counting as in the group (what k_subgroup_affine and
// k_sig_subgroup_g8 do with it)
static bool test_point(const g2j& w) {
  g2a a;
  if (!jac_to_aff(a, w)) return true;
  EXPECT(g2_aff_on_curve(a));
  return g2_aff_in_subgroup_i(a);
}

// runs the kTests tests over the buckets; expect[j]: whether test j must pass.  Returns the batch verdict.
static bool run_tests(const std::vector<g2j>& B, const std::vector<uint32_t>& bits, const std::vector<int>& expect) {
  bool all = true;
  for (uint32_t j = 0; j < kTests; j++) {
    const uint32_t* bj = bits.data() + j;  // one word per test: kBuckets <= 32
    g2j w = jac_infinity<fp2>();
    for (uint32_t l = 0; l < kLanes; l++)
      w = jac_add_i(w, g2_mix_share([&](uint32_t b) { return B[b]; }, bj, l, kLanes, kBuckets));
    const bool ok = test_point(w);
    EXPECT(ok == (expect[j] != 0));
    all = all && ok;
  }
  return all;
}

int main(int argc, char** argv) {
  // ---- the selection, every point of its grid (the Python test holds the expected table)
  for (int ss = 0; ss <= (int)SSUM_BUCKET_MSM; ss++)
    for (int given = 0; given < 2; given++)
      for (int en = 0; en < 2; en++) {
        pipe_batch_plan p;
        p.ssum = (ssum_form)ss;
        pipe_shape s;
        s.scalars_given = given != 0;
        printf("plan %d %d %d %d\n", ss, given, en, (int)pipe_plan_subgroup_batch(p, s, en != 0));
      }
  // ... and it does not look at the rest of the plan or the shape
  {
    pipe_batch_plan p;
    p.subgroup = SUBGROUP_G8, p.alone = true;
    pipe_shape s;
    s.n = 1, s.unblinded = true, s.indexed = true;
    EXPECT(pipe_plan_subgroup_batch(p, s, true));
  }

  std::vector<pt> pts;
  if (argc > 1) pts = load_points(argv[1]);
  const std::vector<g2a> G = of_kind(pts, "g2"), C = of_kind(pts, "curve"), M = of_kind(pts, "mixed"),
                         T13 = of_kind(pts, "ord13"), T23 = of_kind(pts, "ord23");
  if (G.size() < 6 || C.empty() || M.empty() || T13.empty() || T23.empty()) {
    printf("points: %zu (fixture incomplete)\n", pts.size());
    return 1;
  }
  for (const pt& p : pts) EXPECT(g2_aff_on_curve(p.a) && g2_aff_in_subgroup_i(p.a) == (p.in_group != 0));

  std::mt19937 rng(5);
  std::vector<uint32_t> bits(kTests);
  for (uint32_t& w : bits) w = rng() & ((1u << kBuckets) - 1);
  bits[0] = 0;                        // a test that picks nothing: infinity, in the group
  bits[1] = (1u << kBuckets) - 1;     // ... and one that picks every bucket
  auto bit = [&](uint32_t j, uint32_t b) { return (int)((bits[j] >> b) & 1u); };

  // clean buckets: G2 points, an empty bucket (infinity), a repeated point, a point and its negative
  std::vector<std::vector<g2a>> clean(kBuckets);
  for (uint32_t b = 0; b < kBuckets; b++)
    for (uint32_t k = 0; k < b % 5; k++) clean[b].push_back(G[(b + 2 * k) % G.size()]);
  clean[3] = {G[0], G[0], G[1]};
  clean[4] = {G[2], neg(G[2])};
  auto buckets = [&](const std::vector<std::vector<g2a>>& m) {
    std::vector<g2j> B;
    for (const auto& v : m) B.push_back(bucket_of(v));
    return B;
  };
  struct scen {
    const char* name;
    std::vector<std::vector<g2a>> m;
    std::vector<int> expect;
    bool batch;
  };
  std::vector<scen> S;
  auto add = [&](const char* name, const std::vector<std::vector<g2a>>& m, auto&& pass_j) {
    scen s{name, m, std::vector<int>(kTests), true};
    for (uint32_t j = 0; j < kTests; j++) s.batch &= (s.expect[j] = pass_j(j)) != 0;
    S.push_back(s);
  };
  add("all_g2", clean, [&](uint32_t) { return 1; });
  // one dirty bucket: test j fails iff it picks that bucket
  for (const auto& kv : {std::make_pair("one_ord13", T13[0]), std::make_pair("one_ord23", T23[0]),
                         std::make_pair("one_curve", C[0]), std::make_pair("one_mixed", M[0])}) {
    auto m = clean;
    m[7].push_back(kv.second);
    add(kv.first, m, [&](uint32_t j) { return !bit(j, 7); });
  }
  // the dirty point alone in its bucket, and in a bucket that was empty
  {
    auto m = clean;
    m[0] = {T13[1 % T13.size()]};
    add("lone_ord13", m, [&](uint32_t j) { return !bit(j, 0); });
  }
  // T and -T in two buckets: a test passes iff it picks both or neither
  for (const auto& kv : {std::make_pair("pair_ord13", T13[0]), std::make_pair("pair_curve", C[1 % C.size()])}) {
    auto m = clean;
    m[2].push_back(kv.second);
    m[9].push_back(neg(kv.second));
    add(kv.first, m, [&](uint32_t j) { return bit(j, 2) == bit(j, 9); });
  }
  // T + (-T) inside one bucket, adjacent (one chunk: P + (-P) in the mixed addition) and apart (two
  // chunk sums that cancel): clean, every test passes
  {
    auto m = clean;
    m[5] = {T13[0], neg(T13[0]), G[3]};
    m[6] = {C[0], G[4], neg(C[0])};
    add("cancel_in_bucket", m, [&](uint32_t) { return 1; });
  }
  // the same point twice in one bucket (P + P in the mixed addition): 2 T is not zero for odd order
  {
    auto m = clean;
    m[5] = {T23[0], T23[0]};
    add("twice_ord23", m, [&](uint32_t j) { return !bit(j, 5); });
  }
  // ... and 13 times an order-13 point: clean again
  {
    auto m = clean;
    m[8] = std::vector<g2a>(13, T13[0]);
    add("thirteen_ord13", m, [&](uint32_t) { return 1; });
  }
  for (const scen& s : S) {
    const int before = g_bad;
    const bool verdict = run_tests(buckets(s.m), bits, s.expect);
    EXPECT(verdict == s.batch);
    printf("case %s %s %s\n", s.name, verdict ? "pass" : "fail", g_bad == before ? "ok" : "MISMATCH");
  }
  printf("points: %zu  checks: %d  failures: %d\n", pts.size(), g_checks, g_bad);
  return g_bad != 0;
}
