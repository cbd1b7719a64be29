// CPU entry points over the invalid-set search's planner and interpreter (lodestar_amd/csrc/
// lb_search_plan.h) run against the model device of search_model.h: tests/test_search_plan_cpu.py
// drives them over thousands of layouts, tests/test_gpu_parity.py compares the device's search
// trace with what the model predicts.  Built by lodestar_amd/build.py build_search_harness (g++, no HIP).
#include <string.h>

#include "search_model.h"

extern "C" {

// constants of the planner: 0 kWtParts, 1 kSpecMaxSets, 2 kMaxMsm, 3 kMaxRounds
uint32_t c_search_const(uint32_t k) {
  const uint32_t v[4] = {kWtParts, kSpecMaxSets, (uint32_t)kMaxMsm, (uint32_t)kMaxRounds};
  return k < 4 ? v[k] : 0;
}

// One search.  root_of_set[n]: each set's root (0 .. nu - 1, every root used); bad[n]: 1 for a failing
// set; flags: 1 spec_on, 2 r1_plain, 4 rs (per-root sums at hand); lie: search_model.h LIE_*.
// Out: pos_out (<= pos_cap) the positions found mapped to SET indices, in the order found; trace_out
// 5 words per launch set (round, failing nodes, direct checks, weighted tests, form bits); info[0] sets
// found, info[1] launch sets, info[2] rounds entered; msg the violated invariants, one per line.
// Returns the number of violated invariants, or -1 when an output does not fit.
int32_t c_search_run(uint32_t n, uint32_t nu, const uint32_t* root_of_set, const uint8_t* bad, uint32_t flags,
                     uint32_t small_max, int32_t lie, uint32_t* pos_out, uint32_t pos_cap, uint32_t* trace_out,
                     uint32_t trace_cap, uint32_t* info, char* msg, uint32_t msg_cap) {
  search_case c;
  search_layout(c.x, std::vector<uint32_t>(root_of_set, root_of_set + n), nu);
  c.x.rs = (flags & 4u) != 0;
  c.bad.assign(bad, bad + n);
  c.spec_on = (flags & 1u) != 0;
  c.r1_plain = (flags & 2u) != 0;
  c.small_max = small_max;
  c.lie = lie;
  search_result r;
  search_run(c, r);
  info[0] = (uint32_t)r.bad_pos.size();
  info[1] = (uint32_t)(r.trace.size() / 5);
  info[2] = (uint32_t)r.rounds;
  std::string all;
  for (const std::string& s : r.violations) all += s + "\n";
  if (msg_cap) {
    strncpy(msg, all.c_str(), msg_cap - 1);
    msg[msg_cap - 1] = 0;
  }
  if (r.bad_pos.size() > pos_cap || r.trace.size() > trace_cap) return -1;
  for (size_t i = 0; i < r.bad_pos.size(); i++) pos_out[i] = c.x.members[r.bad_pos[i]];
  memcpy(trace_out, r.trace.data(), r.trace.size() * 4);
  return (int32_t)r.violations.size();
}

// blocks of at most 64 over pre[0 .. cnt]: blo, bhi (caller: room for pre[cnt] - pre[0] + cnt each), bo[cnt + 1];
// returns the number of blocks
uint32_t c_blocks64(const uint32_t* pre, uint32_t cnt, uint32_t* blo, uint32_t* bhi, uint32_t* bo) {
  std::vector<uint32_t> l, h, o;
  blocks64(pre, cnt, l, h, o);
  memcpy(blo, l.data(), l.size() * 4);
  memcpy(bhi, h.data(), h.size() * 4);
  memcpy(bo, o.data(), o.size() * 4);
  return (uint32_t)l.size();
}

// failing positions -> jobs: out_job[nj] is updated in place
void c_search_jobs(uint32_t n, const uint32_t* members, const uint32_t* bad_pos, uint32_t n_bad, const uint32_t* job_off,
                   uint32_t nj, int32_t* out_job) {
  search_ctx x;
  x.n = n;
  x.members.assign(members, members + n);
  search_jobs(x, std::vector<uint32_t>(bad_pos, bad_pos + n_bad), std::vector<uint32_t>(job_off, job_off + nj + 1), nj,
              out_job);
}

}  // extern "C"
