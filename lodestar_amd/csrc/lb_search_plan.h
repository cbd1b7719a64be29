// The invalid-set search's host logic (lb_engine.hip search_invalid), device-free: what a round
// launches (the planner) and what its results mean (the interpreter).  No HIP header and nothing
// of the engine: plain C++17 over std::vector, so tests/harness/lb_search_harness.cpp drives the
// same code against a model device on the CPU.  Only lb_engine.hip includes it from the library.
//
// Nodes are ranges of the members array (sets sorted by signing root): subtrees of the root
// product tree (P from the tree), then parts of one root (P = one Miller loop of the part's sum
// r_i PK_i with that root's H(m)).  A failing node carries its FE value y.  Two moves
// (lb_kernels.h k_search_ml / k_search_fe / k_search_match):
//   direct:   each child c of a node gets its own check, y_c = FE(X_c);
//   weighted: one FE of prod_c X_c^(c+1) names the failing child when exactly one fails.
// A failing node descends by a weighted test (one wave for up to 64 children); if the test finds
// two or more failing children, they are checked directly, each failing child in the same round
// getting a weighted test over its own children.  The root starts with direct checks, so one
// round settles two levels.
//
// One round (search_invalid):  search_settle -> work;  per launch set: search_launch_set,
// search_tables (the columns search_round uploads), the device, search_interpret -> next.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

struct snode {
  uint32_t kind;  // 0: node `key` of the root product tree at depth d (d == L: the leaf of root key - mu);
                  // 1: part of root `key`; 2: the single set `key`, checked unblinded
  uint32_t key, lo, len, d;
};
static constexpr uint32_t kYWords = 144;  // an FE value (the k_root_check / k_search_fe layout)
struct fnode {
  snode s;
  bool multi;  // the last weighted test over its children found no single failing child
  std::vector<uint32_t> y;  // FE value (kYWords)
};
struct search_ctx {
  uint32_t n, nu, mu, L;
  std::vector<uint32_t> goff, members;
  bool rs = false;  // the engine's s_root holds the per-root sums S_u
};
struct test_job {
  snode node;
  std::vector<snode> ch;
  bool fresh;    // y from the host (a node failing in an earlier round); else from direct check `d`
  uint32_t src;  // fresh: index into Fs; else index into D
  int32_t spec = -1;    // a look-ahead test of child `spec_k` of fresh test `spec` (y: the parent's)
  uint32_t spec_k = 0;
};
// the search round buffers (lb_engine::sx)
enum {
  SX_KIND, SX_KEY, SX_LO, SX_LEN, SX_MIDX, SX_VERDICT, SX_Y, SX_PK,  // direct checks
  SX_MPRE, SX_MLO, SX_MMODE, SX_MWA, SX_MWB, SX_S,                     // MSM instances
  SX_TMODE, SX_TF, SX_TV0, SX_TU, SX_TMIDX, SX_TYIDX, SX_TLO, SX_TLEN, SX_TPER, SX_TOUT, SX_TPK, SX_YUP,
  SX_ML, SX_BLO, SX_BHI, SX_BO, SX_COUNT
};

// children of a failing node: direct checks fan out to depth max(d + 1, min(d + 7, L - 6)) so a
// weighted test of each failing child can reach the leaves; weighted tests to depth d + 6 (<= 64
// children); a root's members in <= 64 parts for direct checks (one FE each), in <= kWtParts
// parts for a weighted test (one FE whatever f: a root of up to 1024 sets names its failing set
// in one round)
static constexpr uint32_t kWtParts = 1024;  // lb_kernels.h LB_WT_MAX
static inline uint32_t parts_per(uint32_t len, bool direct) {
  const uint32_t f = direct ? 64u : kWtParts;
  return (len + f - 1) / f;
}
// look-ahead tests over the parts of a fresh test's roots (device idle), for nodes of at most this many sets
static constexpr uint32_t kSpecMaxSets = 16384;
static constexpr size_t kMaxMsm = 1024;  // MSM instances per launch set (1280 buckets each)
static constexpr int kMaxRounds = 64;    // depth is bounded far below this
static inline void search_children(const search_ctx& x, const snode& a, bool direct, std::vector<snode>& out) {
  out.clear();
  if (a.kind == 2u || a.len <= 1) return;
  auto parts = [&](uint32_t u, uint32_t lo, uint32_t len) {
    const uint32_t per = parts_per(len, direct);
    for (uint32_t q = 0; q < len; q += per) {
      const uint32_t l = per < len - q ? per : len - q;
      if (l == 1 && direct) out.push_back({2u, x.members[lo + q], lo + q, 1u, 0u});
      else out.push_back({1u, u, lo + q, l, 0u});
    }
  };
  if (a.kind == 1u) return parts(a.key, a.lo, a.len);
  if (a.d == x.L) return parts(a.key - x.mu, a.lo, a.len);
  const int d = (int)a.d, L = (int)x.L;
  // direct children: subtrees of 64 roots (their weighted tests can name one failing root); a
  // node of <= 64 roots whose weighted test matched nothing (>= 2 failing roots) is checked root by
  // root in ONE round (halving it instead took up to six rounds for two wrong roots in a subtree)
  int dd = direct ? (d >= L - 6 ? L : std::max(d + 1, std::min(d + 7, L - 6))) : d + 6;
  if (dd > L) dd = L;
  const uint32_t k = (uint32_t)(dd - d), span = (uint32_t)(L - dd);
  for (uint32_t v = a.key << k; v < (a.key + 1) << k; v++) {
    const uint32_t ulo = (v - (1u << dd)) << span;
    if (ulo >= x.nu) break;
    const uint32_t uhi = std::min(x.nu, ulo + (1u << span));
    out.push_back({0u, v, x.goff[ulo], x.goff[uhi] - x.goff[ulo], (uint32_t)dd});
  }
}

static inline void search_condemn(const snode& a, std::vector<uint32_t>& bad_pos) {
  for (uint32_t q = 0; q < a.len; q++) bad_pos.push_back(a.lo + q);
}

// A round's start: single-child chains and terminals are settled on the host (bad_pos), the
// rest is the round's work.  Past kMaxRounds, fail closed: every node left is condemned whole.
static inline void search_settle(const search_ctx& x, int round, std::vector<fnode>& F, std::vector<fnode>& work,
                                 std::vector<uint32_t>& bad_pos) {
  work.clear();
  if (round > kMaxRounds) {
    for (const fnode& f : F) search_condemn(f.s, bad_pos);
    return;
  }
  std::vector<snode> ch;
  for (fnode& f : F) {
    while (true) {
      if (f.s.len <= 1) {
        bad_pos.push_back(f.s.lo);
        break;
      }
      search_children(x, f.s, f.multi, ch);
      if (ch.size() == 1) {
        f.s = ch[0];
        f.multi = false;
        continue;
      }
      if (ch.empty()) search_condemn(f.s, bad_pos);
      else work.push_back(f);
      break;
    }
  }
}

// One launch set: direct checks D (of the multi nodes' children), then weighted tests: the nodes'
// own fresh tests [0, n_own), their look-ahead tests over roots' parts [n_own, n_fresh) (fresh
// too: y from the host), then the look-ahead tests of the direct checks.
struct launch_set {
  std::vector<fnode> Fs;
  std::vector<snode> D;
  std::vector<uint32_t> d_owner;  // D index -> Fs index
  std::vector<test_job> tests;
  uint32_t n_own = 0, n_fresh = 0;
};
// whole failing nodes from work[a ...] until the MSM instance budget is reached; advances a.
// spec_on: the device runs no other batch; r1_plain: the first round checks subtrees only.
static inline launch_set search_launch_set(const search_ctx& x, const std::vector<fnode>& work, size_t& a, bool spec_on,
                                           bool r1_plain, int round) {
  launch_set ls;
  std::vector<test_job> fresh, spec, ahead;
  size_t inst = 0;
  while (a < work.size() && (ls.Fs.empty() || inst < kMaxMsm)) {
    const fnode& f = work[a++];
    const uint32_t fi = (uint32_t)ls.Fs.size();
    ls.Fs.push_back(f);
    if (!f.multi) {
      test_job t{f.s, {}, true, fi};
      search_children(x, f.s, false, t.ch);
      // a weighted test over <= 64 ROOTS: in the same round, a weighted test over each root's
      // parts, matched against the node's own y (if the node's test names root k, root k is the
      // node's one failing child and y_k = y).  The named root's test then names the set, one
      // round earlier; the other roots' tests are discarded.  Only while the device runs no
      // other batch: under load their Miller loops and final exponentiations cost more than
      // the round they save (profiles/r3_search_spec_ab.txt).
      if (spec_on && !t.ch.empty() && t.ch[0].kind == 0u && t.ch[0].d == x.L && f.s.len <= kSpecMaxSets)
        for (uint32_t k = 0; k < (uint32_t)t.ch.size(); k++) {
          test_job g{t.ch[k], {}, true, fi};
          search_children(x, t.ch[k], false, g.ch);
          if (g.ch.size() < 2) continue;
          g.spec = (int32_t)fresh.size();
          g.spec_k = k;
          spec.push_back(std::move(g));
          inst++;
        }
      fresh.push_back(std::move(t));
      inst++;
      continue;
    }
    std::vector<snode> dch;
    search_children(x, f.s, true, dch);
    for (const snode& c : dch) {
      const uint32_t di = (uint32_t)ls.D.size();
      ls.D.push_back(c);
      ls.d_owner.push_back(fi);
      inst += c.kind != 2u;
      test_job t{c, {}, false, di};
      search_children(x, c, false, t.ch);
      if (t.ch.size() >= 2 && !(r1_plain && round == 1)) {
        ahead.push_back(std::move(t));
        inst++;
      }
    }
  }
  ls.tests = std::move(fresh);
  ls.n_own = (uint32_t)ls.tests.size();
  ls.tests.insert(ls.tests.end(), spec.begin(), spec.end());
  ls.n_fresh = (uint32_t)ls.tests.size();
  ls.tests.insert(ls.tests.end(), ahead.begin(), ahead.end());
  return ls;
}

// A launch set flattened into the columns search_round uploads (col[SX_*]; the buffers the device
// writes stay empty) and the round's form.
struct search_tab {
  std::vector<uint32_t> col[SX_COUNT];
  bool rs_path = false;  // every instance covers whole roots and runs over the per-root sums S_u
  bool w4 = false;       // weight-1 instances only: 32-bit GLV halves, 4 windows instead of 6
  uint32_t cm = 0, T = 0;  // MSM instances, positions they cover (roots when rs_path)
};
static constexpr int kSxUploads[] = {SX_KIND, SX_KEY,   SX_LO,  SX_LEN,  SX_MIDX,  SX_MPRE, SX_MLO,  SX_MMODE, SX_MWA,  SX_MWB,
                                     SX_TMODE, SX_TF,   SX_TV0, SX_TU,   SX_TMIDX, SX_TYIDX, SX_TLO, SX_TLEN,  SX_TPER, SX_YUP};
static inline search_tab search_tables(const search_ctx& x, const std::vector<fnode>& F, const std::vector<snode>& D,
                                       const std::vector<test_job>& tests, uint32_t n_fresh, uint32_t search_small_max) {
  search_tab tab;
  const uint32_t c = (uint32_t)D.size(), nt = (uint32_t)tests.size();
  auto col = [&](int k, uint32_t len) -> std::vector<uint32_t>& {
    tab.col[k].assign(len, 0u);
    return tab.col[k];
  };
  auto &dk = col(SX_KIND, c), &dkey = col(SX_KEY, c), &dlo = col(SX_LO, c), &dlen = col(SX_LEN, c), &dm = col(SX_MIDX, c);
  auto &mlo = tab.col[SX_MLO], &mpre = tab.col[SX_MPRE], &mmode = tab.col[SX_MMODE], &mwa = tab.col[SX_MWA],
       &mwb = tab.col[SX_MWB];
  mpre.assign(1, 0u);
  // the same instances over whole roots (root-level form), while every instance is one
  std::vector<uint32_t> rlo, rpre{0};
  bool root_level = x.rs;
  auto msm = [&](uint32_t lo, uint32_t len, uint32_t mode, uint32_t wa, uint32_t wb, const snode* whole) {
    mlo.push_back(lo);
    mpre.push_back(mpre.back() + len);
    mmode.push_back(mode);
    mwa.push_back(wa);
    mwb.push_back(wb);
    if (whole && whole->kind == 0u) {
      const uint32_t span = x.L - whole->d, ulo = (whole->key - (1u << whole->d)) << span;
      const uint32_t uhi = std::min(x.nu, ulo + (1u << span));
      rlo.push_back(ulo);
      rpre.push_back(rpre.back() + (uhi - ulo));
    } else {
      root_level = false;
    }
    return (uint32_t)mlo.size() - 1;
  };
  for (uint32_t j = 0; j < c; j++) {
    dk[j] = D[j].kind;
    dkey[j] = D[j].key;
    dlo[j] = D[j].lo;
    dlen[j] = D[j].len;
    if (D[j].kind != 2u) dm[j] = msm(D[j].lo, D[j].len, 0u, 1u, 0u, &D[j]);
  }
  auto &tmode = col(SX_TMODE, nt), &tf = col(SX_TF, nt), &tv0 = col(SX_TV0, nt), &tu = col(SX_TU, nt),
       &tm = col(SX_TMIDX, nt), &tyi = col(SX_TYIDX, nt), &tlo = col(SX_TLO, nt), &tlen = col(SX_TLEN, nt),
       &tper = col(SX_TPER, nt);
  auto& yup = col(SX_YUP, kYWords * (n_fresh ? n_fresh : 1));
  for (uint32_t t = 0; t < nt; t++) {
    const test_job& T = tests[t];
    const snode& a = T.node;
    const snode& c0 = T.ch[0];
    tf[t] = (uint32_t)T.ch.size();
    tlo[t] = a.lo;
    tlen[t] = a.len;
    tyi[t] = T.src;
    if (c0.kind == 0u) {  // subtrees of 2^span roots from root ulo0
      const uint32_t span = x.L - c0.d, ulo0 = (c0.key - (1u << c0.d)) << span;
      tmode[t] = 1u;
      tv0[t] = c0.key;
      tm[t] = msm(a.lo, a.len, 1u, ulo0, span, &a);
    } else {  // parts of one root
      const uint32_t per = parts_per(a.len, false);
      tmode[t] = 2u;
      tu[t] = c0.key;
      tper[t] = per;
      tm[t] = msm(a.lo, a.len, 2u, per, 0u, nullptr);
    }
    if (T.fresh) {
      tyi[t] = t;  // fresh tests come first: y_up element t
      for (uint32_t q = 0; q < kYWords; q++) yup[(size_t)q * n_fresh + t] = F[T.src].y[q];
    }
  }
  // root-level round: every instance covers whole roots and the per-set form would take the
  // bucket MSM; the instances then run over the per-root sums S_u (k_rsm_terms)
  tab.rs_path = root_level && !mlo.empty() && mpre.back() > search_small_max;
  if (tab.rs_path) {
    mlo.swap(rlo);
    mpre.swap(rpre);
  }
  tab.w4 = std::all_of(mmode.begin(), mmode.end(), [](uint32_t m) { return m == 0u; });
  tab.cm = (uint32_t)mlo.size();
  tab.T = mpre.back();
  return tab;
}

// Blocks of at most 64 over a prefix array: range j = [pre[j], pre[j + 1]) is tiled by the blocks
// [blo[b], bhi[b]) for b in [bo[j], bo[j + 1]) (k_seg_sum64 sums a block, k_seg_final a range's blocks)
static inline void blocks64(const uint32_t* pre, uint32_t cnt, std::vector<uint32_t>& blo, std::vector<uint32_t>& bhi,
                            std::vector<uint32_t>& bo) {
  blo.clear();
  bhi.clear();
  bo.assign(1, 0u);
  for (uint32_t j = 0; j < cnt; j++) {
    for (uint32_t p = pre[j]; p < pre[j + 1]; p += 64) {
      blo.push_back(p);
      bhi.push_back(std::min(p + 64, pre[j + 1]));
    }
    bo.push_back((uint32_t)blo.size());
  }
}

// What a launch set's results mean: verdict[j] of direct check j (1: passes), ydir the FE values
// (SoA, stride D.size() + tests.size(), direct checks first), tout[t] the child test t matched
// (1-based, 0: none).  Appends the nodes that go on to `next` and what is settled to `bad_pos`.
static inline void search_interpret(const launch_set& ls, const std::vector<int32_t>& verdict,
                                    const std::vector<uint32_t>& ydir, const std::vector<int32_t>& tout,
                                    std::vector<fnode>& next, std::vector<uint32_t>& bad_pos) {
  const std::vector<fnode>& Fs = ls.Fs;
  const std::vector<snode>& D = ls.D;
  const std::vector<test_job>& tests = ls.tests;
  const uint32_t n_own = ls.n_own, n_fresh = ls.n_fresh;
  // fresh tests: the named child (or, by its look-ahead test, the named child's named part),
  // or the node again with its children to check directly
  std::vector<int32_t> spec_of;  // (own test, child) -> look-ahead test
  std::vector<uint32_t> spec_base(n_own + 1, 0);
  for (uint32_t t = n_own; t < n_fresh; t++) spec_base[tests[t].spec + 1]++;
  for (uint32_t t = 0; t < n_own; t++) spec_base[t + 1] += spec_base[t];
  for (uint32_t t = n_own; t < n_fresh; t++) spec_of.push_back((int32_t)t);  // grouped by own test, child order
  for (uint32_t t = 0; t < n_own; t++) {
    const fnode& f = Fs[tests[t].src];
    const int k = tout[t];
    if (k < 1 || (size_t)k > tests[t].ch.size()) {
      next.push_back({f.s, true, f.y});
      continue;
    }
    int32_t st = -1;
    for (uint32_t q = spec_base[t]; q < spec_base[t + 1]; q++)
      if (tests[spec_of[q]].spec_k == (uint32_t)(k - 1)) st = spec_of[q];
    if (st < 0) {
      next.push_back({tests[t].ch[k - 1], false, f.y});
      continue;
    }
    const int k2 = tout[st];
    if (k2 >= 1 && (size_t)k2 <= tests[st].ch.size()) next.push_back({tests[st].ch[k2 - 1], false, f.y});
    else next.push_back({tests[t].ch[k - 1], true, f.y});
  }
  // direct checks: each failing child goes on by its weighted test
  std::vector<int> any_fail(Fs.size(), 0);
  std::vector<int32_t> ahead_of(D.size(), -1);
  for (uint32_t t = n_fresh; t < tests.size(); t++) ahead_of[tests[t].src] = (int32_t)t;
  for (uint32_t j = 0; j < D.size(); j++) {
    if (verdict[j]) continue;
    any_fail[ls.d_owner[j]] = 1;
    std::vector<uint32_t> yc(kYWords);  // y_out is SoA with stride c: gather this node's words
    for (uint32_t q = 0; q < kYWords; q++) yc[q] = ydir[(size_t)q * (D.size() + tests.size()) + j];
    const int32_t t = ahead_of[j];
    if (t < 0) {
      next.push_back({D[j], false, yc});  // terminal or a single child: settled next round
      continue;
    }
    const int k = tout[t];
    if (k >= 1 && (size_t)k <= tests[t].ch.size()) next.push_back({tests[t].ch[k - 1], false, yc});
    else next.push_back({D[j], true, yc});
  }
  // fail closed: a multi node none of whose children fails (impossible for exact arithmetic)
  for (size_t fi = 0; fi < Fs.size(); fi++)
    if (Fs[fi].multi && !any_fail[fi]) search_condemn(Fs[fi].s, bad_pos);
}

// failing positions -> their jobs (set_live makes every failing set belong to a live job): a job
// that was 1 and holds a failing set becomes 0, every other verdict stays
static inline void search_jobs(const search_ctx& x, const std::vector<uint32_t>& bad_pos,
                               const std::vector<uint32_t>& job_off, uint32_t nj, int32_t* out_job) {
  for (uint32_t pos : bad_pos) {
    const uint32_t i = x.members[pos];
    const uint32_t j = (uint32_t)(std::upper_bound(job_off.begin(), job_off.end(), i) - job_off.begin()) - 1;
    if (j < nj && out_job[j] == 1) out_job[j] = 0;
  }
}
