// What the two host units of the library share (lb_engine.hip: the BLS pipeline, whose choice of
// kernel forms is the device-free lb_pipeline_plan.h, the device side and the loop of the
// invalid-set search, whose planning is the device-free lb_search_plan.h, and the small helper calls; lb_kzg_host.hip: the KZG calls): the device buffer, the engine
// and its KZG state, the HIP error macro and the generic "inputs up, one launch, outputs back"
// runner.  Host-only and not part of the public ABI (include/lodestar_bls.h).  Nothing here sits
// in an anonymous namespace: lb_engine must be one type in both units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <mutex>
#include <vector>

#include "lb_fr.h"
#include "lb_kernels.h"
#include "lb_pipeline_plan.h"  // pipe_knobs and the plans (device-free)

struct dbuf {
  void* p = nullptr;
  size_t cap = 0;
  bool view = false;  // p points into another buffer (a batch's upload arena): never freed here
  hipError_t ensure(size_t bytes) {
    if (view) {
      p = nullptr;
      cap = 0;
      view = false;
    }
    if (bytes <= cap) return hipSuccess;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p && !view) hipFree(p);
    p = nullptr;
    cap = 0;
    view = false;
  }
  void set_view(void* q, size_t bytes) {
    if (p && !view) hipFree(p);
    p = q;
    cap = bytes;
    view = true;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// Pipeline stages; (s1) / (s2) = the HIP stream a stage runs on.  s2 carries signature decode,
// pubkey aggregation + blinding and the whole sum(r_i sig_i) branch; s1 groups the sets by
// signing root, hashes each distinct root, sums r_i PK_i per root and runs one Miller loop per
// root into the message product tree.  They join before the root check.  Only a failing root
// runs the per-set fallback (per-set Miller loops + the job tree) and the bisection.
enum {
  ST_DECODE = 0,  // s2
  ST_DEDUP,       // s1
  ST_HASH_MAP,    // s1
  ST_HASH_FIN,    // s1
  ST_PK_CHUNKS,   // s2
  ST_PK_BLIND,    // s2
  ST_SIG_MSM,     // s2
  ST_GSUM,        // s1
  ST_MILLER,      // s1
  ST_TREE_P,      // s1
  ST_ML_S,        // s2
  ST_ROOT,        // s1 (after joining s2)
  ST_FALLBACK,    // s1: invalid-set search, range MSMs + part sums
  ST_BISECT,      // s1: invalid-set search, node checks
  ST_TOTAL,
  kStages
};

// The KZG calls' engine state (lb_kzg_host.hip), all of it set by lb_kzg_load_setup but the FK20 part
struct kzg_state {
  // the trusted setup: [tau^i] G1 as g1a SoA (n entries), [tau^0,1] G2
  dbuf g1, g2;
  uint32_t n = 0;
  // ... and the inverse transform's twiddles for the blob-level calls (lb_fr.h fr_intt_table(12):
  // 2048 powers of the inverse root and 1 / 4096, Montgomery form), built on the host at load
  dbuf tw;
  // ... and, when the setup holds [tau^64] G2 (a third g2a in g2), the cell calls' table (lb_fr.h
  // fr_cell_tables) with the 128 coset factors h_i^64 kept on the host (Montgomery form, by cell index)
  dbuf cell_tab;
  bool cells = false;
  std::vector<fr> h64;
  // FK20 (lb_kzg_compute_cells_and_proofs; lb_fk20.h): the twiddle table of fk_tables and the extended
  // setup X_i[r] (8192 g1j SoA, entry 64 r + i, Jacobian so that O is z = 0), built on the first call
  // under the engine's `mu` and dropped by lb_kzg_load_setup
  dbuf fk_tw, fk_x;
  bool fk_ready = false;
  uint64_t batch_hash_ns = 0;  // host transcript hashing of the last batch verification (lb_kzg_batch_hash_ns)
  void release() {
    for (dbuf* b : {&g1, &g2, &tw, &cell_tab, &fk_tw, &fk_x}) b->release();
  }
};

#ifndef LB_SEARCH_CHUNK_DEF
#define LB_SEARCH_CHUNK_DEF 8
#endif
struct lb_engine {
  int device = 0;
  // LB_ENGINE_LATENCY (lb_engine_create_ex): streams confined to the device's reserved CUs, the
  // latency forms always (the partition keeps every other engine off those CUs)
  bool latency = false;
  int n_cus = 0;  // CUs its streams may use (the whole device, or one side of the partition)
  hipStream_t stream = nullptr;   // s1
  hipStream_t stream2 = nullptr;  // s2
  hipStream_t stream3 = nullptr;  // s3: pubkey aggregation + blinding, beside the signature decode
  hipEvent_t ev_s = nullptr, ev_fork = nullptr, ev_dec = nullptr, ev_pk = nullptr;
  hipEvent_t ev_pkst = nullptr;  // the pubkey statuses (k_pk_blind mode 1), before the ladder
  // small batches alone (round 6): the decoded signatures (s2) -> r_i sig_i on s3 beside the
  // subgroup check (ev_sdec), and the terms ready for the sum on s2 (ev_sblind)
  hipEvent_t ev_sdec = nullptr, ev_sblind = nullptr;
  std::mutex mu;
  // workspace
  dbuf scalars, sig_aff, sig_inf, sig_status, q, h_aff, rpk, pk_status, treeP, treeS, job_status, verdict,
      parts, ok, chunk_acc, chunk_status, fS;
  // message grouping (k_msg_*, k_gsum_*)
  dbuf msg_tab, rep_of, uid_of, uniq_set, n_u, set_uid, gcnt, gpos, goff, gch, chunk_beg, chunk_end, members,
      set_live, gacc, gp_aff, gp_inf, chunk_root;
  // which kernel form each stage takes (lb_pipeline_plan.h): the thresholds and pins, read from the
  // LB_* environment at creation, and the last pipeline run's per-batch plan (per_root_chain, the
  // root check / partial and lb_batch_search_after_partial's root check follow it)
  pipe_knobs knobs;
  pipe_batch_plan plan;
  // bucket MSM for sum r_i sig_i (k_msm_*)
  dbuf sig_aos, bcnt, bcursor, boff, bch, bchunk_beg, bchunk_end, bmembers, bacc, bsum, wsum;
  // The signatures' subgroup check once per batch (lb_pipeline_plan.h pipe_plan_subgroup_batch,
  // k_subgroup_*): LB_SUBGROUP_BATCH=0 turns it off.  sgb_active: the last run_pipeline took it, and
  // its two flag words (sgb_flag) come back with the verdict; a set word reruns the batch with the
  // per-set kernel.  The bits (LB_SGB_TESTS x LB_MSM_NB, from the CSPRNG per run) go up with the
  // scalars; the side chain runs on s3 after the bucket sums (ev_bsum) and joins s1 (ev_sgb).
  bool subgroup_batch = true, sgb_active = false;
  std::vector<uint32_t> h_sgb_bits;
  dbuf sgb_bits, sgb_w, sgb_aff, sgb_inf, sgb_status, sgb_flag;
  hipEvent_t ev_bsum = nullptr, ev_sgb = nullptr;
  uint64_t sgb_runs = 0, sgb_fallbacks = 0;  // lb_subgroup_batch_runs
  // parked lone-lane state: k_hash_finish's points (4 x 72 words per launched lane), k_miller_lane's T
  dbuf park;
  // serial of the batch upload whose lb_batch_partial left its state (trees, statuses, scalars) in
  // this engine's workspace, for lb_batch_search_after_partial; any other pipeline run clears it
  uint64_t partial_serial = 0;
  uint32_t partial_mu = 0;
  // invalid-set search (search_invalid): node descriptors and per-node results
  dbuf sx[32];   // search round buffers (lb_search_plan.h SX_*)
  dbuf pk_aff;  // affine aggregate pubkey per set (single-set checks of the search)
  dbuf y_root;  // FE value of the root check (the search starts from it)
  uint64_t msg_key = 0;  // keyed probe hash (CSPRNG)
  bool hash_row_careful = false;  // LB_HASH_ROW_CAREFUL=1: k_hash_finish_row's exceptional-case path always (tests)
  // one launch pair per search round (look-ahead tests not skipped for passing checks)
  bool search_merge = true;
  dbuf s_terms, s_part;
  // per-root signature sums for the search's root-level instances (LB_SEARCH_ROOTSUM)
  dbuf s_root, rs_idx, s_set;
  bool search_rootsum = true;
  // members per lane in the search rounds' bucket MSM chunks (k_msm_chunks).  Its buckets hold ~8
  // members (109 instances x 1 024 buckets over ~0.9 M entries), so long chunks leave most lanes
  // of a wave idle behind the longest one; LB_SEARCH_CHUNK
  uint32_t search_chunk = LB_SEARCH_CHUNK_DEF;
  // large batches: the first round checks the root tree's top subtrees directly, their S_j from
  // one 4-window bucket MSM over all sets, without look-ahead tests and without the per-root sums
  // (one GLV ladder per set); LB_SEARCH_BLOCKS=0 restores the per-root sums + look-ahead round
  bool search_blk = true;
  // distinct roots numbered in hash-table order (pseudo-random) rather than input order, so the
  // search's first-round subtrees hold comparable numbers of sets (LB_ROOT_SHUFFLE=0: input order)
  bool root_shuffle = true;
  std::vector<uint64_t> h_scalars;
  // resident pubkey table: one 128-byte record per key (g1a + flag, LB_TABLE_REC words)
  dbuf table;
  uint32_t table_n = 0, table_cap = 0;
  // fixed-base comb entries of the table's first comb_n keys (k_comb_fill: LB_COMB_ENTRIES points
  // of 96 B per key, 6.75 KiB), so that r PK of a single-key set is 18 mixed additions
  // (k_pk_blind_comb) instead of the GLV ladder.  comb_max = keys the engine's budget allows:
  // LB_PK_COMB_MB (MiB per engine, default 8192: a 2^20-key table in full), LB_PK_COMB=0 turns
  // the comb off (every set takes the ladder, the A/B).  Keys past the budget take the ladder.
  dbuf comb;
  uint32_t comb_n = 0, comb_cap = 0, comb_max = 0;
  uint64_t comb_sets = 0;  // sets k_pk_blind_comb was launched over, all batches (lb_pubkey_comb_sets)
  kzg_state kzg;
  // lb_block_sets_from_ssz (lb_ssz_sets.h): the upload, the work area (zero-subtree roots, block
  // indices, node and fold scratch) and the packed results, kept between calls; the zero-subtree
  // roots are computed once per work area.  ssz_syncs counts the call's stream synchronisations.
  dbuf ssz_in, ssz_work, ssz_out;
  bool ssz_zh_ready = false;
  std::vector<uint8_t> ssz_up, ssz_down;
  uint64_t ssz_syncs = 0;
  // profiling
  bool profiling = false;
  hipEvent_t ev0[kStages] = {}, ev1[kStages] = {};
  bool used[kStages] = {};
  float last_ms[kStages] = {};
  float acc_ms[kStages] = {};  // stages run once per search round: summed over the rounds
  // pinned host word for the distinct-root count read back after grouping: the per-root kernels
  // are launched over that count, not over the set count (their scratch is sized per dispatch)
  uint32_t* h_nu = nullptr;
  void* h_stage = nullptr;  // pinned staging of small batch uploads (batch_fill, under mu)
  size_t h_stage_cap = 0;
  // engine-owned input workspace reused by lb_verify_jobs* (no per-call device allocation)
  lb_batch* scratch = nullptr;
};

#define LB_HIP(call)                                                                        \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      fprintf(stderr, "lodestar_bls: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(_e), \
              __FILE__, __LINE__);                                                          \
      return LB_ERR_DEVICE;                                                                 \
    }                                                                                       \
  } while (0)

static inline uint32_t nblk(uint32_t n) { return (n + LB_TPB - 1) / LB_TPB; }

// Generic "n items in, per-item outputs back" launcher for the small helper kernels.
struct io_spec {
  const void* src;
  size_t bytes;
  bool out;  // copy back after the launch
  void* dst;
};

template <class Launch>
static int32_t run_simple(lb_engine* e, std::vector<io_spec> io, Launch launch) {
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  std::vector<dbuf> bufs(io.size());
  hipError_t r = hipSuccess;
  for (size_t k = 0; k < io.size() && r == hipSuccess; k++) {
    r = bufs[k].ensure(io[k].bytes ? io[k].bytes : 16);
    if (r == hipSuccess && !io[k].out && io[k].bytes)
      r = hipMemcpyAsync(bufs[k].p, io[k].src, io[k].bytes, hipMemcpyHostToDevice, e->stream);
  }
  if (r == hipSuccess) {
    std::vector<void*> ptrs;
    for (auto& b : bufs) ptrs.push_back(b.p);
    launch(ptrs);
    r = hipGetLastError();
  }
  for (size_t k = 0; k < io.size() && r == hipSuccess; k++)
    if (io[k].out && io[k].dst && io[k].bytes)
      r = hipMemcpyAsync(io[k].dst, bufs[k].p, io[k].bytes, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  for (auto& b : bufs) b.release();
  if (r != hipSuccess) {
    fprintf(stderr, "lodestar_bls: helper kernel failed: %s\n", hipGetErrorString(r));
    return LB_ERR_DEVICE;
  }
  return LB_OK;
}
