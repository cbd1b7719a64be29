// Which kernel form every stage of a batch verification runs: the knobs (thresholds and pins, each
// with its LB_* environment variable), and pure functions from the knobs, the batch's shape and the
// sampled "is the device alone" booleans to small structs of enums.  lb_engine.hip samples
// device_alone() where it always has (the pipeline's start, before the cofactor clearing, before
// the Miller loops, per bucket reduction, per search round), passes the results in and switches on
// what comes back; nothing here reads a clock, a global or the engine.  Device-free (plain g++
// -std=c++17): tests/test_pipeline_plan_cpu.py compares every function with a model of the
// selection as it stood inside run_pipeline, over a grid of knobs and shapes.  The table of
// DESIGN.md section "Form selection" is this file in prose.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// ---------------------------------------------------------------- the knobs
struct pipe_knobs {
  // batches with at most this many distinct roots run their Miller loops one wave per root
  // (k_miller_wave); larger ones one lane per root (k_miller_lane) while other batches are in
  // flight on the device, else 8 lanes per root (k_miller_g8).  LB_MILLER_WAVE_MAX;
  // LB_MILLER_FORM = lane | g8 pins the large-batch form (default: by device load).
  uint32_t miller_wave_max = 2048;
  // ... and up to this many roots (tree nodes of a level, sets of a small batch) on the row engine
  // (lb_row.h: one 16-wave workgroup per item, the products split over 16-lane rows; latency).
  // LB_ROW_MAX.
  uint32_t row_max = 256;
  bool row_fe = true;   // LB_ROW_FE=0 disables the row engine
  int miller_form = 0;  // 0 by load, 1 lane, 2 g8
  // one-lane Miller loops with f and a temporary in LDS (two waves per CU) up to this many roots,
  // f alone in LDS (three waves per CU) above: LB_MILLER_LDS3_MAX (lb_kernels.h k_miller_lane)
  uint32_t miller_lds3_max = 32768;
  // ... and hash_to_G2's cofactor clearing with 8 lanes per root (k_hash_finish_g8).  LB_HASH_G8_MAX.
  uint32_t hash_g8_max = 2048;
  // ... and with a workgroup per root on the row engine while the device is alone.  LB_HASH_ROW_MAX.
  uint32_t hash_row_max = 256;
  // ... and the signature decode's square roots on rows up to this many sets.  LB_DEC_ROW_MAX.
  uint32_t dec_row_max = 4096;
  // ... and the signatures' subgroup check with 8 lanes per set (k_sig_subgroup_g8).  LB_SUBGROUP_G8_MAX.
  uint32_t subgroup_g8_max = 4096;
  // ... and S = sum r_i sig_i by per-set 8-lane scalar multiplications + trees instead of the
  // bucket MSM (k_sig_blind_g8).  LB_SMALL_S_MAX.
  uint32_t small_s_max = 32768;
  uint32_t small_s_g8_max = 2048;  // ... with 8 lanes per set up to here, one lane above (LB_SMALL_S_G8_MAX)
  // bucket sums and the bucket reduction by 8-lane groups (k_msm_buckets_g8, k_msm_window_g8,
  // k_msm_horner_g8); LB_MSM_G8=0: the lone-lane kernels (k_msm_buckets, k_msm_reduce)
  bool msm_g8 = true;
  // the small search rounds' per-position terms: 0 by load (8 lanes per position while the device
  // runs no other batch, one lane under load), 1 one lane, 2 eight lanes (LB_SMSM_FORM=lane / g8)
  int smsm_form = 0;
  // search rounds whose weighted sums cover at most this many positions skip the bucket MSM
  // (k_smsm_terms_g8 + segmented sums).  LB_SEARCH_SMALL_MAX.
  uint32_t search_small_max = 32768;
  int alone_force = -1;  // LB_ALONE=1 / 0 pins device_alone() (tests: the latency forms must run), -1 by load
};

// count: strtoul; flag: atoi != 0; form: "lane" 1, "g8" 2, anything else 0; alone: atoi != 0 ? 1 : 0
enum knob_kind { KNOB_COUNT, KNOB_FLAG, KNOB_FORM, KNOB_ALONE };
struct knob_var {
  const char* name;
  knob_kind kind;
  uint32_t pipe_knobs::*count;
  bool pipe_knobs::*flag;
  int pipe_knobs::*pin;
};
static const knob_var kPipeKnobVars[] = {
    {"LB_MILLER_WAVE_MAX", KNOB_COUNT, &pipe_knobs::miller_wave_max, nullptr, nullptr},
    {"LB_ROW_MAX", KNOB_COUNT, &pipe_knobs::row_max, nullptr, nullptr},
    {"LB_ROW_FE", KNOB_FLAG, nullptr, &pipe_knobs::row_fe, nullptr},
    {"LB_MILLER_LDS3_MAX", KNOB_COUNT, &pipe_knobs::miller_lds3_max, nullptr, nullptr},
    {"LB_MILLER_FORM", KNOB_FORM, nullptr, nullptr, &pipe_knobs::miller_form},
    {"LB_HASH_G8_MAX", KNOB_COUNT, &pipe_knobs::hash_g8_max, nullptr, nullptr},
    {"LB_HASH_ROW_MAX", KNOB_COUNT, &pipe_knobs::hash_row_max, nullptr, nullptr},
    {"LB_DEC_ROW_MAX", KNOB_COUNT, &pipe_knobs::dec_row_max, nullptr, nullptr},
    {"LB_SUBGROUP_G8_MAX", KNOB_COUNT, &pipe_knobs::subgroup_g8_max, nullptr, nullptr},
    {"LB_SMALL_S_MAX", KNOB_COUNT, &pipe_knobs::small_s_max, nullptr, nullptr},
    {"LB_SMALL_S_G8_MAX", KNOB_COUNT, &pipe_knobs::small_s_g8_max, nullptr, nullptr},
    {"LB_SEARCH_SMALL_MAX", KNOB_COUNT, &pipe_knobs::search_small_max, nullptr, nullptr},
    {"LB_SMSM_FORM", KNOB_FORM, nullptr, nullptr, &pipe_knobs::smsm_form},
    {"LB_MSM_G8", KNOB_FLAG, nullptr, &pipe_knobs::msm_g8, nullptr},
    {"LB_ALONE", KNOB_ALONE, nullptr, nullptr, &pipe_knobs::alone_force},
};

// the knobs of an environment (lookup: getenv, or a test's table); an unset variable leaves the default
inline pipe_knobs pipe_knobs_from_env(const char* (*lookup)(const char*)) {
  pipe_knobs k;
  for (const knob_var& v : kPipeKnobVars) {
    const char* s = lookup(v.name);
    if (!s) continue;
    switch (v.kind) {
      case KNOB_COUNT: k.*v.count = (uint32_t)strtoul(s, nullptr, 10); break;
      case KNOB_FLAG: k.*v.flag = atoi(s) != 0; break;
      case KNOB_FORM: k.*v.pin = !strcmp(s, "lane") ? 1 : !strcmp(s, "g8") ? 2 : 0; break;
      case KNOB_ALONE: k.*v.pin = atoi(s) != 0 ? 1 : 0; break;
    }
  }
  return k;
}

// ---------------------------------------------------------------- the forms
enum fe_form { FE_ROW, FE_WAVE };  // one item's Fp12 work: a 16-wave workgroup of rows, or one wave
// per-root sums of r_i PK_i: chunks of LB_GROUP_CHUNK_WAVE members combined by a segmented shuffle
// tree in one launch (k_gsum_wave), or k_gsum_chunks over LB_GROUP_CHUNK members, the chunk sums
// added serially per root
enum gsum_form { GSUM_WAVE, GSUM_CHUNKS };
enum pk_stream { PK_ON_S3, PK_ON_S2 };  // beside the signature decode, or before it
enum pk_chunks_form { PKC_NONE, PKC_INDEXED, PKC_BYTES };
// k_pk_blind in one pass (mode 0); aggregate + status, then the ladder (modes 1, 2); ... the ladder
// by rows (k_pk_blind_rowp); statuses, then the comb over the single-key sets and the ladder over the rest
enum pk_blind_form { PKB_ONE_PASS, PKB_SPLIT, PKB_SPLIT_ROWP, PKB_ROUTE };
enum decode_form { DEC_ROW, DEC_LANE };
enum subgroup_form { SUBGROUP_W4, SUBGROUP_G8, SUBGROUP_LANE };
enum group_form { GROUP_ONE_SET, GROUP_DEVICE_ORDER, GROUP_HOST_ORDER };
// S = sum r_i sig_i: r_i sig_i on s3 beside the subgroup check (k_sig_blind_w4) and the one-workgroup
// sum; one unblinded signature; per-set terms by 8 lanes with the one-workgroup sum; per-set terms by
// one lane with 64:1 levels; the bucket MSM
enum ssum_form { SSUM_PAR_W4, SSUM_UNBLINDED, SSUM_TERMS_G8, SSUM_TERMS_LANE, SSUM_BUCKET_MSM };
enum hash_map_form { HMAP_ROW, HMAP_LANE };
enum hash_fin_form { HFIN_ROW, HFIN_G8, HFIN_LANE };
enum miller_form { MILLER_ROW, MILLER_WAVE, MILLER_LANE3, MILLER_LANE2, MILLER_G8 };
enum msm_buckets_form { MSMB_G8, MSMB_LANE };
enum msm_reduce_form { MSMR_WINDOW_HORNER, MSMR_REDUCE };
enum search_sums_form { SRCH_NO_SUMS, SRCH_TERMS, SRCH_BUCKET_MSM };
enum search_terms_form { STERMS_ROOT_SUMS, STERMS_LANE, STERMS_G8 };

// ---------------------------------------------------------------- per batch
struct pipe_shape {
  uint32_t n = 0;         // sets
  uint32_t n_chunks = 0;  // pubkey aggregation chunks
  uint32_t n_comb = 0;    // single-key sets over a key with comb entries (indexed batches)
  bool indexed = false, routed_here = false;  // ... routed at upload on this engine
  bool scalars_given = false, unblinded = false;
  bool root_shuffle = true;  // lb_engine::root_shuffle
};

struct pipe_batch_plan {
  // `alone` (device_alone at the pipeline's start) picks the latency forms: the row engine's, each
  // up to its own item count (`row`; `row_small`: those over the sets of a small batch), and the
  // per-root sums' wave form
  bool alone = false, row = false, row_small = false;
  gsum_form gsum = GSUM_CHUNKS;
  pk_stream pk_on = PK_ON_S2;
  pk_chunks_form pk_chunks = PKC_NONE;
  pk_blind_form pk_blind = PKB_ONE_PASS;
  decode_form decode = DEC_LANE;
  subgroup_form subgroup = SUBGROUP_LANE;
  group_form group = GROUP_DEVICE_ORDER;
  ssum_form ssum = SSUM_BUCKET_MSM;
  fe_form fe = FE_WAVE;  // ML(-G1, S), the root check, the root partial
};

inline pipe_batch_plan pipe_plan_batch(const pipe_knobs& k, const pipe_shape& s, bool alone) {
  pipe_batch_plan p;
  const uint32_t n = s.n;
  p.alone = alone;
  p.row = alone && k.row_fe;
  p.row_small = p.row && n <= k.row_max;
  p.gsum = alone ? GSUM_WAVE : GSUM_CHUNKS;
  p.fe = p.row ? FE_ROW : FE_WAVE;
  // pubkeys, r*PK: on s3 beside the signature decode for batches up to small_s_max sets (shortens
  // the signature side's chain); on s2 before the decode for large batches, where the two would
  // contend with the per-root chain on s1 for the whole chip (also for a large batch alone on the
  // device: its s1 chain then slowed by more than the s2 chain gained, 5.2 -> 5.1 M sets/s,
  // round-3 A/B)
  p.pk_on = n <= k.small_s_max ? PK_ON_S3 : PK_ON_S2;
  p.pk_chunks = !s.n_chunks ? PKC_NONE : s.indexed ? PKC_INDEXED : PKC_BYTES;
  // on its own stream the pubkey side splits: the aggregates' statuses (what the job statuses and
  // so the S side need) first, then the r PK ladder (only the per-root sums need it).
  // Small batches alone: the ladder with row products, one 16-lane row per set (on s3, before
  // r_i sig_i; a fourth stream per engine, round 6, put 7 engines' 28 streams past what the device
  // schedules without stalls: +10 ms on some batches).
  // An indexed batch routed at upload on this engine, unless the ladder goes by rows: the comb.
  const bool split = p.pk_on == PK_ON_S3;
  if (split && p.row_small) p.pk_blind = PKB_SPLIT_ROWP;
  else if (s.indexed && s.n_comb && s.routed_here) p.pk_blind = PKB_ROUTE;
  else p.pk_blind = split ? PKB_SPLIT : PKB_ONE_PASS;
  p.decode = p.row && n <= k.dec_row_max ? DEC_ROW : DEC_LANE;
  // one wave per signature for a small batch alone (round 6); 8 lanes per signature also for a
  // slot while the device is otherwise idle ran slower: 13.5 vs 13.0 ms per slot,
  // profiles/r3_idle_forms_ab.txt
  p.subgroup = p.row_small ? SUBGROUP_W4 : n <= k.subgroup_g8_max ? SUBGROUP_G8 : SUBGROUP_LANE;
  p.group = n == 1 ? GROUP_ONE_SET : s.root_shuffle ? GROUP_DEVICE_ORDER : GROUP_HOST_ORDER;
  const bool one_unblinded = n == 1 && !s.scalars_given && s.unblinded;
  if (split && !one_unblinded && p.row_small && n <= k.small_s_g8_max) p.ssum = SSUM_PAR_W4;
  else if (one_unblinded) p.ssum = SSUM_UNBLINDED;
  else if (n > k.small_s_max) p.ssum = SSUM_BUCKET_MSM;
  else p.ssum = n <= k.small_s_g8_max ? SSUM_TERMS_G8 : SSUM_TERMS_LANE;
  return p;
}

// The signatures' subgroup check once per batch instead of once per set: the per-set
// kernel of p.subgroup is skipped and LB_SGB_TESTS random 0/1 combinations of the bucket sums take
// Scott's test.  Only on the bucket MSM, whose buckets hold every live signature, and only while
// the engine draws the blinding scalars itself: the digits that place a signature in its buckets
// must be secret from whoever chose the batch.  enabled: LB_SUBGROUP_BATCH (lb_engine::subgroup_batch).
// p.subgroup keeps naming the per-set kernel, which a failing batch test falls back to.
inline bool pipe_plan_subgroup_batch(const pipe_batch_plan& p, const pipe_shape& s, bool enabled) {
  return p.ssum == SSUM_BUCKET_MSM && !s.scalars_given && enabled;
}

// pubkey chunks of <= LB_PK_CHUNK_SMALL keys (a small batch's aggregation is latency) or <= LB_PK_CHUNK
inline bool pipe_pk_chunks_small(const pipe_knobs& k, uint32_t n_sets) { return n_sets <= k.row_max; }

// the row form of a lone Fp12 item outside a pipeline run (lb_fp12_product_is_one)
inline fe_form pipe_fe_form(const pipe_knobs& k, bool alone_now) { return k.row_fe && alone_now ? FE_ROW : FE_WAVE; }

// ---------------------------------------------------------------- per distinct-root count
struct pipe_hash_plan {
  hash_map_form map = HMAP_LANE;
  hash_fin_form fin = HFIN_LANE;
};

// alone_now: device_alone sampled before the cofactor clearing
inline pipe_hash_plan pipe_plan_hash(const pipe_knobs& k, const pipe_batch_plan& b, uint32_t nuh, bool alone_now) {
  pipe_hash_plan p;
  const bool row_hash = b.row && nuh <= k.hash_row_max;  // hash_to_G2 on the row engine
  p.map = row_hash ? HMAP_ROW : HMAP_LANE;
  // 8 lanes per root for few roots, or whenever the device runs no other batch (a few hundred waves
  // on 1 024 SIMDs: latency) unless the Miller form is pinned; one lane per root under load (2.5x
  // less work), as for the Miller loops below
  if (row_hash) p.fin = HFIN_ROW;
  else p.fin = nuh <= k.hash_g8_max || (k.miller_form == 0 && alone_now) ? HFIN_G8 : HFIN_LANE;
  return p;
}

// alone_now: device_alone sampled before the Miller loops
inline miller_form pipe_plan_miller(const pipe_knobs& k, const pipe_batch_plan& b, uint32_t nuh, bool alone_now) {
  if (b.row && nuh <= k.row_max) return MILLER_ROW;
  if (nuh <= k.miller_wave_max) return MILLER_WAVE;
  const bool shared = k.miller_form == 1 || (k.miller_form == 0 && !alone_now);
  if (!shared) return MILLER_G8;
  return nuh <= k.miller_lds3_max ? MILLER_LANE3 : MILLER_LANE2;
}

// a level of `lo` nodes of the root product tree
inline fe_form pipe_tree_form(const pipe_knobs& k, const pipe_batch_plan& b, uint32_t lo) {
  return b.row && lo <= k.row_max ? FE_ROW : FE_WAVE;
}

// ---------------------------------------------------------------- a bucket reduction
struct pipe_msm_plan {
  msm_buckets_form buckets = MSMB_LANE;
  msm_reduce_form reduce = MSMR_REDUCE;
};

// entries: bucket entries (point, window) of the launch, an upper bound; nb buckets; chunk members
// per chunk sum.  The bucket sums go by 8-lane groups (one wave per bucket) only when buckets hold
// several chunks on average (the batch MSM: ~30 chunk sums per bucket); a search round's many small
// instances leave ~one chunk per bucket, which one lane per bucket sums without the wave's idle
// groups.  And only while the device runs no other batch (alone_now): they issue ~6x the
// instructions of one lane per bucket (profiles/r4_r3_valu.txt), which under load is the cost.
inline pipe_msm_plan pipe_plan_msm(const pipe_knobs& k, uint64_t entries, uint32_t chunk, uint32_t nb, bool alone_now) {
  pipe_msm_plan p;
  if (!k.msm_g8) return p;
  p.reduce = MSMR_WINDOW_HORNER;
  p.buckets = entries >= (uint64_t)4 * chunk * nb && alone_now ? MSMB_G8 : MSMB_LANE;
  return p;
}

// ---------------------------------------------------------------- the invalid-set search
struct pipe_search_start {
  bool r1_plain = false;   // the first round checks the root tree's top subtrees directly (lb_engine::search_blk)
  bool root_sums = false;  // per-root signature sums for the root-level instances (lb_engine::search_rootsum)
};

inline pipe_search_start pipe_plan_search_start(const pipe_knobs& k, bool search_blk, bool search_rootsum, uint32_t n,
                                                uint32_t nu) {
  pipe_search_start p;
  const bool large = nu > 1 && n > k.search_small_max;
  p.r1_plain = search_blk && large;
  p.root_sums = !p.r1_plain && search_rootsum && large;
  return p;
}

struct pipe_search_plan {
  search_sums_form sums = SRCH_NO_SUMS;
  search_terms_form terms = STERMS_G8;  // of SRCH_TERMS
};

// cm MSM instances over T positions; rs_path: a root-level round over the per-root sums
// (lb_search_plan.h search_tab); alone_now: device_alone sampled in this round.  A small or
// root-level round: per-position terms + per-instance segmented sums, no bucket MSM.
inline pipe_search_plan pipe_plan_search_round(const pipe_knobs& k, uint32_t cm, uint32_t T, bool rs_path, bool alone_now) {
  pipe_search_plan p;
  if (!cm) return p;
  if (!(T && (rs_path || T <= k.search_small_max))) {
    p.sums = SRCH_BUCKET_MSM;
    return p;
  }
  p.sums = SRCH_TERMS;
  if (rs_path) p.terms = STERMS_ROOT_SUMS;
  else p.terms = k.smsm_form == 1 || (k.smsm_form == 0 && !alone_now) ? STERMS_LANE : STERMS_G8;
  return p;
}
