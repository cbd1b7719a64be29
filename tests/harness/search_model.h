// The invalid-set search on the CPU: the planner and interpreter of lodestar_amd/csrc/lb_search_plan.h
// driven by the loop of lb_engine.hip search_invalid against a MODEL DEVICE, with the invariants of
// every launch set's tables checked on the way.  Shared by lb_search_harness.cpp (the entry points
// tests/test_search_plan_cpu.py calls) and tests/native/search_plan_check.cpp (the sanitizer program).
//
// The model: a layout (n sets over nu roots: goff, members) and the failing sets `bad`.  An FE value
// y stands for the bad positions of the node it came from; its first two words carry that node's
// lo, len.  It reads what the device reads -- the uploaded columns -- not the planner's structures:
//   * a direct check passes iff the range its MSM instance sums holds no bad position (kind 2: iff
//     set `key` is good), and returns y = (lo, len) of the checked node;
//   * a weighted test of node a against y returns k iff the bad positions of a are those y stands
//     for, there is one, and every one has weight k (mode 1: ((root - wa) >> wb) + 1, mode 2:
//     (position - lo) / per + 1), k <= f; else 0.  The device under exact arithmetic.
// Lies (fail-closed behaviour): LIE_PASS every direct check passes; LIE_TOUT every test returns an
// out-of-range child; LIE_STALL the round's results are dropped and the same nodes fail again.
#pragma once
#include <stdio.h>

#include <string>

#include "lb_search_plan.h"

enum { LIE_NONE = 0, LIE_PASS, LIE_TOUT, LIE_STALL };

struct search_case {
  search_ctx x;               // n, nu, mu, L, goff, members, rs
  std::vector<uint8_t> bad;   // by set index
  bool spec_on = false, r1_plain = false;
  uint32_t small_max = 32768;
  int lie = LIE_NONE;
};
struct search_result {
  std::vector<uint32_t> bad_pos;
  std::vector<uint32_t> trace;  // per launch set: round, failing nodes, direct checks, weighted tests, form bits
                                // (1 rs_path, 2 w4, 4 no bucket MSM)
  int rounds = 0;               // rounds entered (kMaxRounds + 1: the limit condemned what was left)
  std::vector<std::string> violations;
};

struct search_model {
  const search_case& c;
  search_result& r;
  std::vector<uint32_t> pre;     // pre[p] = bad positions below p
  std::vector<uint32_t> root_of;  // position -> root
  explicit search_model(const search_case& c_, search_result& r_) : c(c_), r(r_) {
    const search_ctx& x = c.x;
    pre.assign(x.n + 1, 0);
    for (uint32_t p = 0; p < x.n; p++) pre[p + 1] = pre[p] + (c.bad[x.members[p]] ? 1u : 0u);
    root_of.resize(x.n);
    for (uint32_t u = 0; u < x.nu; u++)
      for (uint32_t p = x.goff[u]; p < x.goff[u + 1]; p++) root_of[p] = u;
  }
  void fail(int round, const char* what, uint32_t a = 0, uint32_t b = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, "round %d: %s (%u, %u)", round, what, a, b);
    if (r.violations.size() < 32) r.violations.push_back(buf);
  }
  uint32_t cnt(uint32_t lo, uint32_t hi) const { return hi > lo ? pre[hi] - pre[lo] : 0; }
  uint32_t first_bad(uint32_t lo) const {  // the first bad position >= lo (one exists)
    return (uint32_t)(std::upper_bound(pre.begin(), pre.end(), pre[lo]) - pre.begin()) - 1;
  }
  uint32_t last_bad(uint32_t hi) const {  // the last bad position < hi (one exists)
    return (uint32_t)(std::lower_bound(pre.begin(), pre.end(), pre[hi]) - pre.begin()) - 1;
  }
  // the member range instance m sums: [lo, hi)
  void inst_range(const search_tab& t, uint32_t m, uint32_t& lo, uint32_t& hi) const {
    const uint32_t a = t.col[SX_MLO][m], len = t.col[SX_MPRE][m + 1] - t.col[SX_MPRE][m];
    if (t.rs_path) {
      lo = c.x.goff[a];
      hi = c.x.goff[a + len];
    } else {
      lo = a;
      hi = a + len;
    }
  }

  void check_tables(int round, const launch_set& ls, const search_tab& t) {
    const search_ctx& x = c.x;
    const uint32_t nc = (uint32_t)ls.D.size(), nt = (uint32_t)ls.tests.size();
    const auto& mpre = t.col[SX_MPRE];
    const auto& mmode = t.col[SX_MMODE];
    if (mpre.empty() || mpre[0] != 0) return fail(round, "mpre does not start at 0");
    for (size_t j = 1; j < mpre.size(); j++)
      if (mpre[j] < mpre[j - 1]) fail(round, "mpre decreases", (uint32_t)j);
    if (t.cm != t.col[SX_MLO].size() || t.cm + 1 != mpre.size() || t.T != mpre.back() || mmode.size() != t.cm ||
        t.col[SX_MWA].size() != t.cm || t.col[SX_MWB].size() != t.cm)
      return fail(round, "cm / T do not describe the instance columns", t.cm, t.T);
    for (int k : {SX_KIND, SX_KEY, SX_LO, SX_LEN, SX_MIDX})
      if (t.col[k].size() != nc) return fail(round, "a direct-check column has not one entry per check", (uint32_t)k);
    for (int k : {SX_TMODE, SX_TF, SX_TV0, SX_TU, SX_TMIDX, SX_TYIDX, SX_TLO, SX_TLEN, SX_TPER})
      if (t.col[k].size() != nt) return fail(round, "a test column has not one entry per test", (uint32_t)k);
    if (t.w4 != std::all_of(mmode.begin(), mmode.end(), [](uint32_t m) { return m == 0u; }))
      fail(round, "w4 is not 'every instance mode is 0'");
    if (t.rs_path && !(x.rs && t.cm && t.T <= x.nu * t.cm)) fail(round, "rs_path without per-root sums");
    // every instance sums exactly the node's member range (through goff in the root-level form)
    auto covers = [&](uint32_t m, uint32_t lo, uint32_t len, const char* what, uint32_t i) {
      if (m >= t.cm) return fail(round, what, i, m);
      if (t.rs_path && t.col[SX_MLO][m] + (mpre[m + 1] - mpre[m]) > x.nu) return fail(round, "root range past nu", i, m);
      if (!t.rs_path && t.col[SX_MLO][m] + (mpre[m + 1] - mpre[m]) > x.n) return fail(round, "member range past n", i, m);
      uint32_t ilo, ihi;
      inst_range(t, m, ilo, ihi);
      if (ilo != lo || ihi != lo + len) fail(round, "an instance does not sum its node's member range", i, m);
    };
    uint32_t used = 0;
    for (uint32_t j = 0; j < nc; j++) {
      const snode& d = ls.D[j];
      if (t.col[SX_KIND][j] != d.kind || t.col[SX_KEY][j] != d.key || t.col[SX_LO][j] != d.lo || t.col[SX_LEN][j] != d.len)
        fail(round, "direct-check columns differ from D", j);
      if (d.kind == 2u) {
        if (d.len != 1 || d.lo >= x.n || x.members[d.lo] != d.key) fail(round, "kind 2 is not the set at its position", j);
        continue;
      }
      covers(t.col[SX_MIDX][j], d.lo, d.len, "dm index not below cm", j);
      used++;
    }
    if (ls.n_own > ls.n_fresh || ls.n_fresh > nt) fail(round, "n_own <= n_fresh <= tests does not hold");
    if (t.col[SX_YUP].size() != (size_t)kYWords * (ls.n_fresh ? ls.n_fresh : 1)) fail(round, "yup size");
    for (uint32_t i = 0; i < nt; i++) {
      const test_job& tj = ls.tests[i];
      const uint32_t f = t.col[SX_TF][i], md = t.col[SX_TMODE][i], m = t.col[SX_TMIDX][i];
      if (tj.fresh != (i < ls.n_fresh)) fail(round, "fresh tests do not precede look-ahead tests", i);
      if ((tj.spec >= 0) != (i >= ls.n_own && i < ls.n_fresh) || (tj.spec >= 0 && (uint32_t)tj.spec >= ls.n_own))
        fail(round, "a look-ahead test over parts does not name an own test", i);
      if (tj.fresh ? tj.src >= ls.Fs.size() : tj.src >= nc) fail(round, "a test's y source is out of range", i);
      if (f != tj.ch.size() || f < 2 || f > (md == 2u ? kWtParts : 64u)) fail(round, "children of a weighted test", i, f);
      covers(m, tj.node.lo, tj.node.len, "tm index not below cm", i);
      used++;
      if (m >= t.cm) continue;
      if (mmode[m] != md) fail(round, "test and instance modes differ", i);
      if (i < ls.n_fresh) {
        if (t.col[SX_TYIDX][i] != i) fail(round, "a fresh test's y index is not its own", i);
        if (tj.src < ls.Fs.size())
          for (uint32_t q = 0; q < kYWords; q++)
            if (t.col[SX_YUP][(size_t)q * ls.n_fresh + i] != ls.Fs[tj.src].y[q]) {
              fail(round, "yup does not hold the owner's y", i, q);
              break;
            }
      } else if (t.col[SX_TYIDX][i] != tj.src) {
        fail(round, "a look-ahead test's y index is not its direct check", i);
      }
      // the children the device weighs are the planner's children, in order
      for (uint32_t k = 0; k < f && k < tj.ch.size(); k++) {
        uint32_t lo, hi;
        child_range(t, i, k, lo, hi);
        if (lo != tj.ch[k].lo || hi != tj.ch[k].lo + tj.ch[k].len || tj.ch[k].len == 0) {
          fail(round, "weights do not split the node into the planner's children", i, k);
          break;
        }
        if (md == 1u && tj.ch[k].key != t.col[SX_TV0][i] + k) fail(round, "tree children are not v0 + k", i, k);
        if (md == 2u && tj.ch[k].key != t.col[SX_TU][i]) fail(round, "parts of another root", i, k);
      }
    }
    if (used != t.cm) fail(round, "instances nobody reads", used, t.cm);
    // the launch set exceeds the instance budget only by its last whole node
    if (ls.Fs.size() > 1) {
      const uint32_t last = (uint32_t)ls.Fs.size() - 1;
      uint32_t li = 0;
      for (uint32_t j = 0; j < nc; j++) li += ls.d_owner[j] == last && ls.D[j].kind != 2u;
      for (const test_job& tj : ls.tests) li += tj.fresh ? tj.src == last : ls.d_owner[tj.src] == last;
      if (t.cm - li >= kMaxMsm) fail(round, "over the instance budget before the last node", t.cm, li);
    }
  }
  // child k of test i by the weights the device computes: mode 1 roots [wa + (k << wb), wa + ((k + 1) << wb))
  // of the node, mode 2 positions [lo + k per, lo + (k + 1) per) of the node
  void child_range(const search_tab& t, uint32_t i, uint32_t k, uint32_t& lo, uint32_t& hi) const {
    const uint32_t m = t.col[SX_TMIDX][i], wa = t.col[SX_MWA][m], wb = t.col[SX_MWB][m];
    uint32_t alo, ahi;
    inst_range(t, m, alo, ahi);
    if (t.col[SX_TMODE][i] == 1u) {
      const uint32_t ulo = std::min(c.x.nu, wa + (k << wb)), uhi = std::min(c.x.nu, wa + ((k + 1) << wb));
      lo = std::max(alo, c.x.goff[ulo]);
      hi = std::min(ahi, c.x.goff[uhi]);
    } else {
      lo = std::min(ahi, alo + k * wa);
      hi = std::min(ahi, alo + (k + 1) * wa);
    }
    if (hi < lo) hi = lo;
  }

  // the device: verdict, ydir (SoA, stride c + nt), tout
  void run(const launch_set& ls, const search_tab& t, std::vector<int32_t>& verdict, std::vector<uint32_t>& ydir,
           std::vector<int32_t>& tout) {
    const uint32_t nc = (uint32_t)ls.D.size(), nt = (uint32_t)ls.tests.size(), N = nc + nt;
    verdict.assign(nc, 1);
    ydir.assign((size_t)kYWords * N, 0u);
    tout.assign(nt, 0);
    for (uint32_t j = 0; j < nc; j++) {
      bool pass;
      if (t.col[SX_KIND][j] == 2u) {
        pass = !c.bad[t.col[SX_KEY][j]];
      } else {
        uint32_t lo, hi;
        inst_range(t, t.col[SX_MIDX][j], lo, hi);
        pass = cnt(lo, hi) == 0;
      }
      verdict[j] = (pass || c.lie == LIE_PASS) ? 1 : 0;
      ydir[(size_t)0 * N + j] = t.col[SX_LO][j];
      ydir[(size_t)1 * N + j] = t.col[SX_LEN][j];
    }
    for (uint32_t i = 0; i < nt; i++) {
      if (c.lie == LIE_TOUT) {
        tout[i] = (i & 1u) ? -7 : (int32_t)t.col[SX_TF][i] + 1;
        continue;
      }
      uint32_t ylo, ylen;
      if (i < ls.n_fresh) {
        ylo = t.col[SX_YUP][(size_t)0 * ls.n_fresh + i];
        ylen = t.col[SX_YUP][(size_t)1 * ls.n_fresh + i];
      } else {
        const uint32_t j = t.col[SX_TYIDX][i];
        if (verdict[j]) continue;  // y = 1: no match
        ylo = ydir[(size_t)0 * N + j];
        ylen = ydir[(size_t)1 * N + j];
      }
      uint32_t alo, ahi;
      inst_range(t, t.col[SX_TMIDX][i], alo, ahi);
      const uint32_t nb = cnt(alo, ahi), ilo = std::max(alo, ylo), ihi = std::min(ahi, ylo + ylen);
      if (!nb || nb != cnt(ylo, ylo + ylen) || nb != cnt(ilo, ihi)) continue;  // other bad positions than y's
      const uint32_t p0 = first_bad(alo), p1 = last_bad(ahi);
      const uint32_t m = t.col[SX_TMIDX][i], wa = t.col[SX_MWA][m], wb = t.col[SX_MWB][m];
      auto weight = [&](uint32_t p) {
        return t.col[SX_TMODE][i] == 1u ? ((root_of[p] - wa) >> wb) + 1u : (p - alo) / wa + 1u;
      };
      if (weight(p0) == weight(p1) && weight(p0) <= t.col[SX_TF][i]) tout[i] = (int32_t)weight(p0);
    }
  }
};

// the loop of lb_engine.hip search_invalid, the model in place of search_round
static inline void search_run(const search_case& c, search_result& r) {
  const search_ctx& x = c.x;
  search_model dev(c, r);
  fnode root{{0u, 1u, 0u, x.n, 0u}, true, std::vector<uint32_t>(kYWords, 0u)};
  root.y[1] = x.n;
  std::vector<fnode> F{root}, work;
  for (int round = 1; !F.empty(); round++) {
    r.rounds = round;
    const std::vector<fnode> before(F);
    std::vector<fnode> next;
    search_settle(x, round, F, work, r.bad_pos);
    for (size_t a = 0; a < work.size();) {
      const launch_set ls = search_launch_set(x, work, a, c.spec_on, c.r1_plain, round);
      const search_tab tab = search_tables(x, ls.Fs, ls.D, ls.tests, ls.n_fresh, c.small_max);
      dev.check_tables(round, ls, tab);
      if (!r.violations.empty()) return;  // the model reads the tables: not past a broken one
      std::vector<int32_t> verdict, tout;
      std::vector<uint32_t> ydir;
      dev.run(ls, tab, verdict, ydir, tout);
      const bool small = tab.cm && tab.T && (tab.rs_path || tab.T <= c.small_max);
      for (uint32_t v : {(uint32_t)round, (uint32_t)ls.Fs.size(), (uint32_t)ls.D.size(), (uint32_t)ls.tests.size(),
                         (tab.rs_path ? 1u : 0u) | (tab.w4 ? 2u : 0u) | (small ? 4u : 0u)})
        r.trace.push_back(v);
      search_interpret(ls, verdict, ydir, tout, next, r.bad_pos);
    }
    if (c.lie == LIE_STALL && round <= kMaxRounds) next = before;
    F.swap(next);
  }
}

// a layout from each set's root (roots numbered 0 .. nu - 1, every one used): members in set order
static inline void search_layout(search_ctx& x, const std::vector<uint32_t>& root_of_set, uint32_t nu) {
  x.n = (uint32_t)root_of_set.size();
  x.nu = nu;
  x.mu = 1;
  while (x.mu < nu) x.mu <<= 1;
  x.L = 0;
  while ((1u << x.L) < x.mu) x.L++;
  x.goff.assign(nu + 1, 0);
  for (uint32_t u : root_of_set) x.goff[u + 1]++;
  for (uint32_t u = 0; u < nu; u++) x.goff[u + 1] += x.goff[u];
  std::vector<uint32_t> cur(x.goff.begin(), x.goff.end() - 1);
  x.members.assign(x.n, 0);
  for (uint32_t i = 0; i < x.n; i++) x.members[cur[root_of_set[i]]++] = i;
}
