// CPU entry points over the batch pipeline's form selection (lodestar_amd/csrc/lb_pipeline_plan.h):
// tests/test_pipeline_plan_cpu.py compares them with its own model of the selection over a grid of
// knobs and shapes.  Knobs travel as int64 values in the order of kPipeKnobVars; every plan
// function is evaluated over arrays of points, one output byte per plan field.
// Built by lodestar_amd/build.py build_pipeline_harness (g++, no HIP).
#include <map>
#include <string>

#include "lb_pipeline_plan.h"

namespace {
constexpr uint32_t kVars = sizeof(kPipeKnobVars) / sizeof(kPipeKnobVars[0]);

pipe_knobs knobs_of(const int64_t* v) {
  pipe_knobs k;
  for (uint32_t i = 0; i < kVars; i++) {
    const knob_var& d = kPipeKnobVars[i];
    if (d.count) k.*d.count = (uint32_t)v[i];
    if (d.flag) k.*d.flag = v[i] != 0;
    if (d.pin) k.*d.pin = (int)v[i];
  }
  return k;
}

void knobs_out(const pipe_knobs& k, int64_t* v) {
  for (uint32_t i = 0; i < kVars; i++) {
    const knob_var& d = kPipeKnobVars[i];
    v[i] = d.count ? (int64_t)(k.*d.count) : d.flag ? (int64_t)(k.*d.flag) : (int64_t)(k.*d.pin);
  }
}

std::map<std::string, std::string> g_env;
const char* env_lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
}  // namespace

extern "C" {

uint32_t c_pipe_knob_count(void) { return kVars; }
const char* c_pipe_knob_name(uint32_t i) { return i < kVars ? kPipeKnobVars[i].name : ""; }
void c_pipe_knob_defaults(int64_t* out) { knobs_out(pipe_knobs(), out); }

// the knobs of the environment `text`: NAME=VALUE lines
void c_pipe_env(const char* text, int64_t* out) {
  g_env.clear();
  const std::string s(text);
  for (size_t a = 0; a < s.size();) {
    size_t b = s.find('\n', a);
    if (b == std::string::npos) b = s.size();
    const size_t eq = s.find('=', a);
    if (eq != std::string::npos && eq < b) g_env[s.substr(a, eq - a)] = s.substr(eq + 1, b - eq - 1);
    a = b + 1;
  }
  knobs_out(pipe_knobs_from_env(env_lookup), out);
}

// flags: 1 indexed, 2 routed on this engine, 4 scalars given, 8 unblinded, 16 root_shuffle, 32 alone.
// out, 12 bytes per point: alone row row_small gsum pk_on pk_chunks pk_blind decode subgroup group ssum fe
void c_pipe_batch(const int64_t* knobs, uint32_t m, const uint32_t* n, const uint32_t* n_chunks, const uint32_t* n_comb,
                  const uint8_t* flags, uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    const uint8_t f = flags[i];
    const pipe_shape s{n[i], n_chunks[i], n_comb[i], (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0, (f & 16) != 0};
    const pipe_batch_plan p = pipe_plan_batch(k, s, (f & 32) != 0);
    const uint8_t row[12] = {p.alone, p.row, p.row_small, (uint8_t)p.gsum, (uint8_t)p.pk_on, (uint8_t)p.pk_chunks,
                             (uint8_t)p.pk_blind, (uint8_t)p.decode, (uint8_t)p.subgroup, (uint8_t)p.group,
                             (uint8_t)p.ssum, (uint8_t)p.fe};
    memcpy(out + 12 * (size_t)i, row, 12);
  }
}

// The per-root functions of a batch of n sets whose pipeline started with `alone` = flags & 1;
// flags & 2: the sample before the cofactor clearing, flags & 4: the sample before the Miller loops.
// out, 4 bytes per point: hash map, cofactor clearing, Miller loop, the tree level of `lo` nodes
void c_pipe_roots(const int64_t* knobs, uint32_t m, const uint32_t* n, const uint32_t* nuh, const uint32_t* lo,
                  const uint8_t* flags, uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    pipe_shape s;
    s.n = n[i];
    const pipe_batch_plan b = pipe_plan_batch(k, s, (flags[i] & 1) != 0);
    const pipe_hash_plan h = pipe_plan_hash(k, b, nuh[i], (flags[i] & 2) != 0);
    out[4 * (size_t)i + 0] = (uint8_t)h.map;
    out[4 * (size_t)i + 1] = (uint8_t)h.fin;
    out[4 * (size_t)i + 2] = (uint8_t)pipe_plan_miller(k, b, nuh[i], (flags[i] & 4) != 0);
    out[4 * (size_t)i + 3] = (uint8_t)pipe_tree_form(k, b, lo[i]);
  }
}

// out, 2 bytes per point: bucket sums, reduction
void c_pipe_msm(const int64_t* knobs, uint32_t m, const uint64_t* entries, const uint32_t* chunk, const uint32_t* nb,
                const uint8_t* alone_now, uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    const pipe_msm_plan p = pipe_plan_msm(k, entries[i], chunk[i], nb[i], alone_now[i] != 0);
    out[2 * (size_t)i + 0] = (uint8_t)p.buckets;
    out[2 * (size_t)i + 1] = (uint8_t)p.reduce;
  }
}

// flags: 1 rs_path, 2 alone_now.  out, 2 bytes per point: sums, terms
void c_pipe_search_round(const int64_t* knobs, uint32_t m, const uint32_t* cm, const uint32_t* T, const uint8_t* flags,
                         uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    const pipe_search_plan p = pipe_plan_search_round(k, cm[i], T[i], (flags[i] & 1) != 0, (flags[i] & 2) != 0);
    out[2 * (size_t)i + 0] = (uint8_t)p.sums;
    out[2 * (size_t)i + 1] = (uint8_t)p.terms;
  }
}

// flags: 1 search_blk, 2 search_rootsum.  out, 2 bytes per point: r1_plain, root_sums
void c_pipe_search_start(const int64_t* knobs, uint32_t m, const uint32_t* n, const uint32_t* nu, const uint8_t* flags,
                         uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    const pipe_search_start p = pipe_plan_search_start(k, (flags[i] & 1) != 0, (flags[i] & 2) != 0, n[i], nu[i]);
    out[2 * (size_t)i + 0] = p.r1_plain;
    out[2 * (size_t)i + 1] = p.root_sums;
  }
}

// out, 3 bytes per point: small pubkey chunks for n sets, the lone Fp12 item's form while alone / under load
void c_pipe_misc(const int64_t* knobs, uint32_t m, const uint32_t* n, uint8_t* out) {
  const pipe_knobs k = knobs_of(knobs);
  for (uint32_t i = 0; i < m; i++) {
    out[3 * (size_t)i + 0] = pipe_pk_chunks_small(k, n[i]);
    out[3 * (size_t)i + 1] = (uint8_t)pipe_fe_form(k, true);
    out[3 * (size_t)i + 2] = (uint8_t)pipe_fe_form(k, false);
  }
}

}  // extern "C"
