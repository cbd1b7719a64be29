// C-ABI engine (include/lodestar_bls.h) driving the gfx950 pipeline of lb_kernels.h.
//
// One engine per GPU, one HIP stream per engine; calls on one engine are serialised by a
// mutex (the reference's worker pool runs one job package per worker at a time,
// multithread/index.ts:290-381).  Inputs are copied into device memory at batch creation
// (the reference structured-clones its BlsWorkReq[], multithread/index.ts:330), so the
// caller never has to keep its buffers alive.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "lb_kernels.h"
#include "lb_engine_impl.h"  // dbuf, lb_engine, LB_HIP, run_simple: shared with lb_kzg_host.hip (the KZG calls)
#include "lb_kdecl.h"  // kernels of the other translation units (split build)
#include "lb_search_plan.h"  // the invalid-set search's planner and interpreter (device-free)
// (lb_pipeline_plan.h, every stage's kernel form, comes with lb_engine_impl.h: lb_engine holds its knobs)

#define LB_ABI_VERSION 1

namespace {
const char* const kStageNames[kStages] = {"decode_sigs", "dedup",   "hash_map", "hash_finish", "pk_chunks",
                                          "pk_blind",    "sig_msm", "group_sum", "miller",    "tree_up_P",
                                          "ml_S",        "root_check", "search_msm", "search_check", "total"};

}  // namespace

struct lb_batch {
  uint32_t n_jobs = 0, n_sets = 0, n_pks = 0;
  // unique per upload (batch_fill): lb_batch_search_after_partial matches on it, not on the
  // address, which a freed batch's successor may reuse
  uint64_t serial = 0;
  std::vector<uint32_t> job_off;  // host copy (bisection bookkeeping)
  std::vector<uint32_t> h_set_chunk_off, h_chunk_lo;  // host staging of the chunk decomposition
  uint32_t n_chunks = 0;           // pubkey aggregation chunks (k_pk_chunks)
  bool indexed = false;            // pubkeys are indices into the engine's resident table
  // r PK routing of an indexed batch (batch_fill): d_route = the set ids of the single-key sets
  // whose key had comb entries at upload, [0, n_comb), then every other set (the ladder's),
  // [n_comb, n_sets).  Valid on route_eng only (the comb table is per engine; its coverage never
  // shrinks, so keys covered at upload stay covered).
  std::vector<uint32_t> h_route;
  uint32_t n_comb = 0;
  const void* route_eng = nullptr;
  dbuf d_job_off, d_pk_off, d_pks, d_msgs, d_sigs, d_sig_sizes, d_set_chunk_off, d_chunk_lo, d_route;
  dbuf d_arena;  // small uploads: the arrays above as views into one buffer, filled by one copy
  bool has_sizes = false;
  int device = 0;
  ~lb_batch() {
    d_job_off.release();
    d_arena.release();
    d_pk_off.release();
    d_pks.release();
    d_msgs.release();
    d_sigs.release();
    d_sig_sizes.release();
    d_set_chunk_off.release();
    d_chunk_lo.release();
    d_route.release();
  }
};

// Engines per device are capped so that one process cannot create more concurrently active
// HIP streams than the device can back with queues and scratch (exhaustion aborts the HSA queue
// asynchronously instead of returning an error).  LB_MAX_ENGINES_PER_DEVICE overrides the cap.
// Round 4: 7 -> 10.  Every queue's scratch is reserved for the largest private segment it runs
// times the device's wave capacity; with the per-root kernels at <= 2.7 KB per lane (k_miller_lane
// was 6.7 KB) 8 and 10 engines run without an abort (profiles/r4_engines_ab.txt), and
// lb_engine_create reserves each engine's s1 scratch up front (above).
static std::mutex g_engine_mu;
static int g_engine_count[64];
static std::atomic<uint64_t> g_batch_serial{0};
// Batches currently inside the pipeline per device (all engines of the process).  With more than
// one, the device is throughput-bound and the per-root kernels take their work-efficient forms.
static std::atomic<int> g_device_busy[64];
// The two most recent pipeline exits per device by distinct engines (steady-clock ns): exit[0] the
// latest, exit[1] the latest of any other engine than exit[0]'s, so an engine can ask when ANOTHER
// engine last left the pipeline (round-4 ADVICE: one slot let an engine that left 1 ms after
// another see the device as idle while the other was between two batches)
struct exit_rec {
  const void* eng = nullptr;
  int64_t ns = 0;
};
static std::mutex g_exit_mu[64];
static exit_rec g_device_exit[64][2];
static int64_t lb_now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// CUs reserved for latency engines per device (0: no partition); engines created while a
// partition exists run on the complement.  LB_LATENCY_CUS (default 8 of the device's CUs).  The
// partition lives as long as a latency engine does (g_latency_live counts them): after the last
// one is destroyed, engines created later get the whole device again (round-5 ADVICE).
static int g_latency_cus[64];
static int g_latency_live[64];
struct busy_scope {
  int dev;
  const void* eng;
  bool counted;
  busy_scope(int d, const void* e, bool latency = false) : dev(d), eng(e), counted(!latency) {
    if (counted) g_device_busy[dev].fetch_add(1, std::memory_order_relaxed);
  }
  ~busy_scope() {
    if (!counted) return;  // a latency engine's calls run on its own CUs: not load for the others
    {
      std::lock_guard<std::mutex> lk(g_exit_mu[dev]);
      exit_rec* r = g_device_exit[dev];
      if (r[0].eng != eng) r[1] = r[0];
      r[0] = exit_rec{eng, lb_now_ns()};
    }
    g_device_busy[dev].fetch_sub(1, std::memory_order_relaxed);
  }
};
// The device runs no other batch: none inside the pipeline, and no OTHER engine's batch left it
// within the last LB_ALONE_GRACE_MS (an in-flight engine's host thread between two batches is
// still load: at 7 in flight those gaps sent batches to the latency forms, ~2 % of the headline,
// profiles/r4_regress_ab.txt)
#ifndef LB_ALONE_GRACE_MS
#define LB_ALONE_GRACE_MS 20
#endif
template <class E>
static bool device_alone(const E* e) {
  if (e->latency) return true;  // its reserved CUs run nothing else
  if (e->knobs.alone_force >= 0) return e->knobs.alone_force != 0;
  if (g_device_busy[e->device].load(std::memory_order_relaxed) > 1) return false;
  int64_t other;
  {
    std::lock_guard<std::mutex> lk(g_exit_mu[e->device]);
    const exit_rec* r = g_device_exit[e->device];
    other = r[0].eng != (const void*)e ? r[0].ns : r[1].ns;
  }
  return other == 0 || lb_now_ns() - other > (int64_t)LB_ALONE_GRACE_MS * 1000000;
}
static int max_engines_per_device() {
  const char* v = getenv("LB_MAX_ENGINES_PER_DEVICE");
  int k = v ? atoi(v) : 0;
  return k > 0 ? k : 10;  // the highest engine count measured abort-free (profiles/r4_engines_ab.txt)
}

static inline uint32_t nblk_inv(uint32_t n) { return (n + LB_INV_TPB - 1) / LB_INV_TPB; }

// unblinded: the verdict of this run covers exactly this batch (lb_batch_verify / lb_verify_jobs*),
// so a 1-set batch may verify unblinded as Signature.verify does.  A partial product that is
// multiplied with other ranks' partials (lb_batch_partial) is always blinded: two unblinded 1-set
// partials sig_A + D and sig_B - D would cancel in the product (round-5 ADVICE).
static int fill_scalars(lb_engine* e, uint32_t n, const uint64_t* user, bool unblinded) {
  e->h_scalars.resize(n);
  if (!user && n == 1 && unblinded) {
    e->h_scalars[0] = 1;  // one set: verified unblinded (k_sig_unblinded), as Signature.verify
    return LB_OK;
  }
  if (user) {
    for (uint32_t i = 0; i < n; i++)
      if (user[i] == 0) return LB_BAD_SCALAR;
    memcpy(e->h_scalars.data(), user, (size_t)n * 8);
  } else {
    // blst verifyMultipleSignatures: 8 bytes from the CSPRNG per set, forced non-zero
    size_t need = (size_t)n * 8, got = 0;
    uint8_t* dst = reinterpret_cast<uint8_t*>(e->h_scalars.data());
    while (got < need) {
      ssize_t r = getrandom(dst + got, need - got, 0);
      if (r < 0) return LB_ERR_DEVICE;
      got += (size_t)r;
    }
    for (uint32_t i = 0; i < n; i++)
      while (e->h_scalars[i] == 0) getrandom(&e->h_scalars[i], 8, 0);
  }
  return LB_OK;
}

extern "C" {

int32_t lb_abi_version(void) { return LB_ABI_VERSION; }

const char* lb_error_name(int32_t code) {
  switch (code) {
    case LB_OK: return "BLST_SUCCESS";
    case LB_BAD_ENCODING: return "BLST_BAD_ENCODING";
    case LB_POINT_NOT_ON_CURVE: return "BLST_POINT_NOT_ON_CURVE";
    case LB_POINT_NOT_IN_GROUP: return "BLST_POINT_NOT_IN_GROUP";
    case LB_AGGR_TYPE_MISMATCH: return "BLST_AGGR_TYPE_MISMATCH";
    case LB_VERIFY_FAIL: return "BLST_VERIFY_FAIL";
    case LB_PK_IS_INFINITY: return "BLST_PK_IS_INFINITY";
    case LB_BAD_SCALAR: return "BLST_BAD_SCALAR";
    case LB_INVALID_SIZE: return "BLST_INVALID_SIZE";
    case LB_EMPTY_AGGREGATE_ARRAY: return "EMPTY_AGGREGATE_ARRAY";
    case LB_EMPTY_SIGNATURE_SET: return "Empty signature set";
    case LB_ERR_ARGUMENT: return "LB_ERR_ARGUMENT";
    case LB_ERR_DEVICE: return "LB_ERR_DEVICE";
    case LB_ERR_NO_DEVICE: return "LB_ERR_NO_DEVICE";
    default: return "LB_UNKNOWN_ERROR";
  }
}

// the leading run of gfx950 ordinals (lb_engine_create_ex refuses any other device, and ordinals
// from 64 up: the per-device tables above)
int32_t lb_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return 0;
  int n = 0;
  for (; n < count && n < 64; n++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, n) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;
  }
  return n;
}

int32_t lb_engine_create(int32_t device, lb_engine** out) { return lb_engine_create_ex(device, 0u, out); }
// a CU mask over [lo, hi) of ncu CUs (32 per word)
static std::vector<uint32_t> cu_mask(int ncu, int lo, int hi) {
  std::vector<uint32_t> m((size_t)(ncu + 31) / 32, 0u);
  for (int c = lo; c < hi && c < ncu; c++) m[(size_t)c / 32] |= 1u << (c % 32);
  return m;
}
int32_t lb_engine_create_ex(int32_t device, uint32_t flags, lb_engine** out) {
  if (!out || (flags & ~LB_ENGINE_LATENCY)) return LB_ERR_ARGUMENT;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return LB_ERR_NO_DEVICE;
  if (device < 0) LB_HIP(hipGetDevice(&device));
  if (device >= count) return LB_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  LB_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "lodestar_bls: device %d is %s, this build targets gfx950 only\n", device, prop.gcnArchName);
    return LB_ERR_NO_DEVICE;
  }
  LB_HIP(hipSetDevice(device));
  if (device >= 64) return LB_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(g_engine_mu);
    if (g_engine_count[device] >= max_engines_per_device()) {
      fprintf(stderr, "lodestar_bls: engine limit (%d per device) reached on device %d\n", max_engines_per_device(),
              device);
      return LB_ERR_DEVICE;
    }
    g_engine_count[device]++;
  }
  lb_engine* e = new lb_engine();
  e->device = device;
  while (getrandom(&e->msg_key, 8, 0) != 8) {
  }
  // s1 carries the latency-bound chain (grouping, per-root hashing and Miller loops, the root
  // check, the invalid-set search), created at the least stream priority as measured: the
  // greatest priority for it cost the headline 2-3 % and did not help the search (round 3,
  // profiles/r3_search_split_ab.txt)
  int prio_least = 0, prio_greatest = 0;
  hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  e->knobs = pipe_knobs_from_env([](const char* name) -> const char* { return getenv(name); });
  if (const char* hc = getenv("LB_HASH_ROW_CAREFUL")) e->hash_row_careful = std::atoi(hc) != 0;
  if (const char* sm = getenv("LB_SEARCH_MERGE")) e->search_merge = std::atoi(sm) != 0;
  if (const char* sm = getenv("LB_SEARCH_ROOTSUM")) e->search_rootsum = std::atoi(sm) != 0;
  if (const char* sc = getenv("LB_SEARCH_CHUNK")) {
    const uint32_t v = (uint32_t)strtoul(sc, nullptr, 10);
    if (v >= 1 && v <= 64) e->search_chunk = v;
  }
  if (const char* sm = getenv("LB_SEARCH_BLOCKS")) e->search_blk = std::atoi(sm) != 0;
  if (const char* sm = getenv("LB_ROOT_SHUFFLE")) e->root_shuffle = std::atoi(sm) != 0;
  if (const char* sb = getenv("LB_SUBGROUP_BATCH")) e->subgroup_batch = std::atoi(sb) != 0;
  {
    const char* on = getenv("LB_PK_COMB");
    const char* mb = getenv("LB_PK_COMB_MB");
    const double mib = mb ? std::max(0.0, strtod(mb, nullptr)) : 8192.0;  // fractions allowed (tests)
    const uint64_t keys = (uint64_t)(mib * 1048576.0 / (double)(LB_COMB_ENTRIES * sizeof(g1a)));
    e->comb_max = (on && std::atoi(on) == 0) ? 0u : (uint32_t)std::min<uint64_t>(keys, 0x7fffffffu);
  }
  // CU partition: a latency engine's streams on the reserved CUs [0, R), every engine created
  // while a partition exists on [R, ncu)
  bool masked = false;
  std::vector<uint32_t> mask;
  {
    std::lock_guard<std::mutex> lk(g_engine_mu);
    const int ncu = prop.multiProcessorCount;
    e->n_cus = ncu;
    if (flags & LB_ENGINE_LATENCY) {
      if (g_latency_cus[device] == 0) {
        const char* v = getenv("LB_LATENCY_CUS");
        const int r = v ? atoi(v) : 8;
        g_latency_cus[device] = std::max(1, std::min(r, ncu / 4));
        // engines created before the partition keep the whole device (their streams exist):
        // they share the reserved CUs, which only costs the latency engine its isolation
        if (g_engine_count[device] > 1)
          fprintf(stderr, "lodestar_bls: latency engine created after %d other engine(s) on device %d: "
                  "those still run on every CU (create the latency engine first)\n", g_engine_count[device] - 1, device);
      }
      g_latency_live[device]++;
      e->latency = true;
      mask = cu_mask(ncu, 0, g_latency_cus[device]);
      e->n_cus = g_latency_cus[device];
      masked = true;
    } else if (g_latency_cus[device] > 0) {
      mask = cu_mask(ncu, g_latency_cus[device], ncu);
      e->n_cus = ncu - g_latency_cus[device];
      masked = true;
    }
  }
  auto mk = [&](hipStream_t* st, bool prio) {
    if (masked) return hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data());
    return prio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_least)
                : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  };
  if (mk(&e->stream, true) != hipSuccess || mk(&e->stream2, false) != hipSuccess || mk(&e->stream3, false) != hipSuccess ||
      hipHostMalloc((void**)&e->h_nu, 4, hipHostMallocDefault) != hipSuccess) {
    if (e->stream) hipStreamDestroy(e->stream);
    if (e->stream2) hipStreamDestroy(e->stream2);
    if (e->stream3) hipStreamDestroy(e->stream3);
    std::lock_guard<std::mutex> lk(g_engine_mu);
    g_engine_count[device]--;
    if (e->latency && --g_latency_live[device] == 0) g_latency_cus[device] = 0;
    delete e;
    return LB_ERR_DEVICE;
  }
  hipEventCreateWithFlags(&e->ev_s, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_dec, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_pk, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_pkst, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_sdec, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_sblind, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_bsum, hipEventDisableTiming);
  hipEventCreateWithFlags(&e->ev_sgb, hipEventDisableTiming);
  for (int i = 0; i < kStages; i++) {
    hipEventCreate(&e->ev0[i]);
    hipEventCreate(&e->ev1[i]);
  }
  // Reserve the streams' scratch now, one engine at a time, for the largest private segments the
  // forms of lb_pipeline_plan.h can put on them: empty dispatches over more waves than the device
  // holds.  s1: MILLER_LANE2 (k_miller_lane<2>, 2.7 KB per lane) and HFIN_LANE (k_hash_finish).
  // The runtime sizes a queue's scratch for the largest segment it has run, from one per-process
  // pool, and a queue that cannot grow it mid-run aborts asynchronously; growing it here, with the
  // stream synchronised, turns an exhausted pool into LB_ERR_DEVICE from lb_engine_create.
  {
    bool ok;
    {
      std::lock_guard<std::mutex> lk(g_engine_mu);
      ok = e->n_u.ensure(4) == hipSuccess && hipMemsetAsync(e->n_u.p, 0, 4, e->stream) == hipSuccess;
      if (ok) {
        hipLaunchKernelGGL(k_miller_lane<2>, dim3(4096), dim3(LB_TPB), 0, e->stream, 0u, 1u, e->n_u.as<uint32_t>(),
                           nullptr, nullptr, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(k_hash_finish, dim3(4096), dim3(LB_INV_TPB), 0, e->stream, 0u, e->n_u.as<uint32_t>(),
                           nullptr, nullptr, nullptr, 0u);
        // s2 and s3 the same way (round 6), each for the forms with a private segment it runs,
        // at their largest dispatch.  s2: DEC_LANE, the signature decode over the whole device
        // (472 B per lane), and below SUBGROUP_G8 and SSUM_TERMS_G8 (616 / 868 B), whose largest
        // dispatches are their knobs.  s3: PKC_BYTES, the 96-byte-key chunk sums (584 B), and
        // PKB_SPLIT_ROWP.  The other forms of s2 / s3 need less per lane and fewer lanes (resource
        // table: DESIGN.md section 5.2).
        const pipe_knobs& k = e->knobs;
        hipLaunchKernelGGL(k_decompress_sigs, dim3(4096), dim3(LB_TPB), 0, e->stream2, 0u, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(k_pk_chunks, dim3(4096), dim3(LB_TPB), 0, e->stream3, 0u, nullptr, nullptr, nullptr, nullptr);
        // the row r PK ladder (one row per set), at the largest small batch: row_max sets
        hipLaunchKernelGGL(k_pk_blind_rowp, dim3(std::max<uint32_t>(1u, k.row_max)), dim3(64), 0, e->stream3,
                           0u, nullptr, nullptr, nullptr, nullptr);
        // (one wave per 8 sets, at least one wave, at most 16 384: more than the device holds)
        auto g8_waves = [](uint32_t sets) { return dim3(std::min<uint32_t>(16384u, std::max<uint32_t>(1u, sets / 8 + 1))); };
        hipLaunchKernelGGL(k_sig_subgroup_g8, g8_waves(k.subgroup_g8_max), dim3(64), 0, e->stream2, 0u, nullptr,
                           nullptr, nullptr);
        hipLaunchKernelGGL(k_sig_blind_g8, g8_waves(k.small_s_g8_max), dim3(64), 0, e->stream2, 0u, nullptr, nullptr,
                           nullptr, nullptr, nullptr);
        // s3 also carries the per-batch subgroup test of a bucket-MSM batch (its pubkey work is on
        // s2 then): k_subgroup_mix's out-of-line additions over LB_SGB_TESTS waves, SUBGROUP_G8 over
        // the LB_SGB_TESTS mixed points
        hipLaunchKernelGGL(k_subgroup_mix, dim3(LB_SGB_TESTS), dim3(64), 0, e->stream3, nullptr, 0u, nullptr, nullptr);
        hipLaunchKernelGGL(k_subgroup_affine, dim3(1), dim3(LB_INV_TPB), 0, e->stream3, 0u, nullptr, nullptr, nullptr,
                           nullptr);
        hipLaunchKernelGGL(k_sig_subgroup_g8, dim3(LB_SGB_TESTS / 8), dim3(64), 0, e->stream3, 0u, nullptr, nullptr,
                           nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess &&
             hipStreamSynchronize(e->stream2) == hipSuccess && hipStreamSynchronize(e->stream3) == hipSuccess;
      }
    }
    if (!ok) {
      fprintf(stderr, "lodestar_bls: engine scratch reservation failed on device %d\n", device);
      lb_engine_destroy(e);
      return LB_ERR_DEVICE;
    }
  }
  *out = e;
  return LB_OK;
}

void lb_engine_destroy(lb_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  dbuf* bufs[] = {&e->scalars, &e->sig_aff, &e->sig_inf, &e->sig_status, &e->q, &e->h_aff, &e->rpk,
                  &e->pk_status, &e->treeP, &e->treeS, &e->job_status, &e->verdict, &e->parts,
                  &e->ok, &e->chunk_acc, &e->chunk_status, &e->fS, &e->table, &e->comb, &e->msg_tab,
                  &e->rep_of, &e->uid_of, &e->uniq_set, &e->n_u, &e->set_uid, &e->gcnt, &e->gpos, &e->goff,
                  &e->gch, &e->chunk_beg, &e->chunk_end, &e->members, &e->set_live, &e->gacc, &e->gp_aff,
                  &e->gp_inf, &e->chunk_root, &e->sig_aos, &e->bcnt, &e->bcursor, &e->boff, &e->bch, &e->bchunk_beg,
                  &e->bchunk_end, &e->bmembers, &e->bacc, &e->bsum, &e->wsum, &e->park, &e->pk_aff, &e->y_root,
                  &e->s_terms, &e->s_part, &e->s_root, &e->rs_idx, &e->s_set, &e->sgb_bits, &e->sgb_w, &e->sgb_aff,
                  &e->sgb_inf, &e->sgb_status, &e->sgb_flag, &e->ssz_in, &e->ssz_work, &e->ssz_out};
  for (dbuf* b : bufs) b->release();
  e->kzg.release();
  for (dbuf& b : e->sx) b.release();
  for (int i = 0; i < kStages; i++) {
    if (e->ev0[i]) hipEventDestroy(e->ev0[i]);
    if (e->ev1[i]) hipEventDestroy(e->ev1[i]);
  }
  hipEventDestroy(e->ev_s);
  hipEventDestroy(e->ev_fork);
  hipEventDestroy(e->ev_dec);
  hipEventDestroy(e->ev_pk);
  if (e->ev_pkst) hipEventDestroy(e->ev_pkst);
  if (e->ev_sdec) hipEventDestroy(e->ev_sdec);
  if (e->ev_sblind) hipEventDestroy(e->ev_sblind);
  if (e->ev_bsum) hipEventDestroy(e->ev_bsum);
  if (e->ev_sgb) hipEventDestroy(e->ev_sgb);
  hipStreamSynchronize(e->stream2);
  hipStreamSynchronize(e->stream3);
  if (e->scratch) delete e->scratch;
  if (e->h_nu) hipHostFree(e->h_nu);
  if (e->h_stage) hipHostFree(e->h_stage);
  hipStreamDestroy(e->stream2);
  hipStreamDestroy(e->stream3);
  hipStreamDestroy(e->stream);
  {
    std::lock_guard<std::mutex> lk(g_engine_mu);
    g_engine_count[e->device]--;
    if (e->latency && --g_latency_live[e->device] == 0) g_latency_cus[e->device] = 0;
  }
  delete e;
}

int32_t lb_engine_cu_count(const lb_engine* e) { return e ? e->n_cus : 0; }

int32_t lb_engine_set_profiling(lb_engine* e, int32_t enable) {
  if (!e) return LB_ERR_ARGUMENT;
  e->profiling = enable != 0;
  return LB_OK;
}

int32_t lb_engine_last_profile(lb_engine* e, const char** names, float* ms, int32_t cap, int32_t* n) {
  if (!e || !n) return LB_ERR_ARGUMENT;
  int k = cap < kStages ? cap : kStages;
  for (int i = 0; i < k; i++) {
    if (names) names[i] = kStageNames[i];
    if (ms) ms[i] = e->last_ms[i];
  }
  *n = k;
  return LB_OK;
}

}  // extern "C"

// Validates the offsets and uploads one batch into b's device buffers (grown, never shrunk, so
// an engine-owned workspace batch is reused across calls without device allocation).  The caller
// holds e->mu.
static constexpr size_t kStageMax = (size_t)1 << 20;  // batch uploads up to this go up as one copy
static int32_t batch_fill(lb_engine* e, lb_batch* b, uint32_t n_jobs, const uint32_t* job_offsets,
                          const uint32_t* set_pk_offsets, const uint8_t* pubkeys, const uint32_t* pk_indices,
                          const uint8_t* signing_roots, const uint8_t* signatures, const uint32_t* sig_sizes) {
  if (!e || !job_offsets || !set_pk_offsets) return LB_ERR_ARGUMENT;
  if (job_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t j = 0; j < n_jobs; j++)
    if (job_offsets[j + 1] < job_offsets[j]) return LB_ERR_ARGUMENT;
  const uint32_t n_sets = job_offsets[n_jobs];
  if (set_pk_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t i = 0; i < n_sets; i++)
    if (set_pk_offsets[i + 1] < set_pk_offsets[i]) return LB_ERR_ARGUMENT;
  const uint32_t n_pks = set_pk_offsets[n_sets];
  if (n_pks & LB_CHUNK_FIRST) return LB_ERR_ARGUMENT;  // key offsets are 31-bit (chunk flags)
  const bool indexed = pk_indices != nullptr;
  if ((n_sets && (!signing_roots || !signatures)) || (n_pks && !pubkeys && !indexed)) return LB_ERR_ARGUMENT;
  LB_HIP(hipSetDevice(e->device));
  b->device = e->device;
  b->serial = g_batch_serial.fetch_add(1, std::memory_order_relaxed) + 1;
  b->n_jobs = n_jobs;
  b->n_sets = n_sets;
  b->n_pks = n_pks;
  b->job_off.assign(job_offsets, job_offsets + n_jobs + 1);
  b->has_sizes = sig_sizes != nullptr;
  auto up = [&](dbuf& d, const void* src, size_t bytes) -> hipError_t {
    hipError_t r = d.ensure(bytes ? bytes : 16);
    if (r != hipSuccess || !bytes) return r;
    return hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, e->stream);
  };
  // chunk decomposition of every set's pubkey range (<= LB_PK_CHUNK keys per chunk; a small batch,
  // whose aggregation is latency -- a block's 131 sets of ~256 keys --, <= LB_PK_CHUNK_SMALL: its
  // serial chain per lane 16 -> 4 mixed additions before the six-level segmented tree)
  std::vector<uint32_t>& set_chunk_off = b->h_set_chunk_off;
  std::vector<uint32_t>& chunk_lo = b->h_chunk_lo;
  set_chunk_off.resize(n_sets + 1);
  chunk_lo.clear();
  const uint32_t pkc = pipe_pk_chunks_small(e->knobs, n_sets) ? LB_PK_CHUNK_SMALL : LB_PK_CHUNK;
  for (uint32_t i = 0; i < n_sets; i++) {
    set_chunk_off[i] = (uint32_t)chunk_lo.size();
    for (uint32_t k = set_pk_offsets[i]; k < set_pk_offsets[i + 1]; k += pkc)
      chunk_lo.push_back(k | (k == set_pk_offsets[i] ? LB_CHUNK_FIRST : 0u));  // flag: the set's first chunk
  }
  set_chunk_off[n_sets] = (uint32_t)chunk_lo.size();
  b->n_chunks = (uint32_t)chunk_lo.size();
  chunk_lo.push_back(n_pks | LB_CHUNK_FIRST);  // chunk c ends where chunk c+1 starts (chunks never
  // span sets: a set's last chunk ends at the next set's first key, which is its own first chunk start)
  b->indexed = indexed;
  // r PK routing (run_pipeline): single-key sets over a key with comb entries first, the rest after
  std::vector<uint32_t>& route = b->h_route;
  route.clear();
  b->n_comb = 0;
  b->route_eng = nullptr;
  if (indexed && e->comb_n) {
    route.resize(n_sets);
    uint32_t lo = 0, hi = n_sets;
    for (uint32_t i = n_sets; i-- > 0;)  // the ladder sets from the back, in ascending order
      if (!(set_pk_offsets[i + 1] - set_pk_offsets[i] == 1 && pk_indices[set_pk_offsets[i]] < e->comb_n))
        route[--hi] = i;
    for (uint32_t i = 0; i < n_sets; i++)
      if (set_pk_offsets[i + 1] - set_pk_offsets[i] == 1 && pk_indices[set_pk_offsets[i]] < e->comb_n)
        route[lo++] = i;
    b->n_comb = lo;
    b->route_eng = e;
  }
  struct part {
    dbuf* d;
    const void* src;
    size_t bytes;
  };
  const part parts[] = {{&b->d_job_off, job_offsets, (size_t)(n_jobs + 1) * 4},
                        {&b->d_set_chunk_off, set_chunk_off.data(), set_chunk_off.size() * 4},
                        {&b->d_chunk_lo, chunk_lo.data(), chunk_lo.size() * 4},
                        {&b->d_pk_off, set_pk_offsets, (size_t)(n_sets + 1) * 4},
                        {&b->d_pks, indexed ? (const void*)pk_indices : (const void*)pubkeys,
                         (size_t)n_pks * (indexed ? 4 : 96)},
                        {&b->d_msgs, signing_roots, (size_t)n_sets * 32},
                        {&b->d_sigs, signatures, (size_t)n_sets * 96},
                        {&b->d_sig_sizes, sig_sizes, sig_sizes ? (size_t)n_sets * 4 : 0},
                        {&b->d_route, route.data(), route.size() * 4}};
  // a small batch (a 1-set call, a block) goes up as ONE copy from pinned staging into an arena
  // the arrays are views of: one pageable copy per array were ~0.1 ms of a 1-set call's 3.7
  size_t total = 0;
  for (const part& q : parts) total += ((q.bytes > 16 ? q.bytes : 16) + 255) & ~(size_t)255;
  bool staged = total <= kStageMax;
  if (staged && e->h_stage_cap < total) {
    if (e->h_stage) hipHostFree(e->h_stage);
    e->h_stage = nullptr;
    e->h_stage_cap = 0;
    if (hipHostMalloc(&e->h_stage, kStageMax, hipHostMallocDefault) == hipSuccess) e->h_stage_cap = kStageMax;
    else staged = false;
  }
  hipError_t r = hipSuccess;
  if (staged) {
    r = b->d_arena.ensure(total);
    size_t off = 0;
    for (const part& q : parts) {
      if (q.bytes) memcpy(static_cast<uint8_t*>(e->h_stage) + off, q.src, q.bytes);
      off += ((q.bytes > 16 ? q.bytes : 16) + 255) & ~(size_t)255;
    }
    if (r == hipSuccess) r = hipMemcpyAsync(b->d_arena.p, e->h_stage, total, hipMemcpyHostToDevice, e->stream);
    off = 0;
    for (const part& q : parts) {
      const size_t sz = ((q.bytes > 16 ? q.bytes : 16) + 255) & ~(size_t)255;
      if (r == hipSuccess && (q.bytes || q.d != &b->d_sig_sizes)) q.d->set_view(static_cast<uint8_t*>(b->d_arena.p) + off, sz);
      off += sz;
    }
  } else {
    for (const part& q : parts)
      if (r == hipSuccess && (q.bytes || q.d != &b->d_sig_sizes)) r = up(*q.d, q.src, q.bytes);
  }
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r != hipSuccess) {
    // no view may outlive a failed (re)allocation of the arena: the batch is left empty, so a
    // later verify of it reads nothing (round-5 ADVICE)
    for (const part& q : parts) q.d->release();
    b->d_arena.release();
    b->n_jobs = b->n_sets = b->n_pks = b->n_chunks = b->n_comb = 0;
    b->job_off.assign(1, 0u);
    fprintf(stderr, "lodestar_bls: batch upload failed: %s\n", hipGetErrorString(r));
    return LB_ERR_DEVICE;
  }
  return LB_OK;
}

static int32_t batch_create(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets, const uint32_t* set_pk_offsets,
                            const uint8_t* pubkeys, const uint32_t* pk_indices, const uint8_t* signing_roots,
                            const uint8_t* signatures, const uint32_t* sig_sizes, lb_batch** out) {
  if (!e || !out) return LB_ERR_ARGUMENT;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(e->mu);
  lb_batch* b = new lb_batch();
  int32_t st = batch_fill(e, b, n_jobs, job_offsets, set_pk_offsets, pubkeys, pk_indices, signing_roots, signatures,
                          sig_sizes);
  if (st != LB_OK) {
    delete b;
    return st;
  }
  *out = b;
  return LB_OK;
}

// pk_indices == NULL is only meaningful when no set carries a key (every set then rejects with
// EMPTY_AGGREGATE_ARRAY); it is passed on as a one-word sentinel, never read.
static const uint32_t kNoIndices[1] = {0};
static int32_t check_null_indices(uint32_t n_jobs, const uint32_t* job_offsets, const uint32_t* set_pk_offsets) {
  if (!job_offsets || !set_pk_offsets) return LB_ERR_ARGUMENT;
  return set_pk_offsets[job_offsets[n_jobs]] == 0 ? LB_OK : LB_ERR_ARGUMENT;
}

extern "C" {

int32_t lb_batch_create(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets, const uint32_t* set_pk_offsets,
                        const uint8_t* pubkeys, const uint8_t* signing_roots, const uint8_t* signatures,
                        const uint32_t* sig_sizes, lb_batch** out) {
  return batch_create(e, n_jobs, job_offsets, set_pk_offsets, pubkeys, nullptr, signing_roots, signatures, sig_sizes,
                      out);
}

int32_t lb_batch_create_indexed(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                                const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                                const uint8_t* signing_roots, const uint8_t* signatures, const uint32_t* sig_sizes,
                                lb_batch** out) {
  if (!pk_indices) {
    const int32_t st = check_null_indices(n_jobs, job_offsets, set_pk_offsets);
    if (st != LB_OK) return st;
    pk_indices = kNoIndices;
  }
  return batch_create(e, n_jobs, job_offsets, set_pk_offsets, nullptr, pk_indices, signing_roots, signatures,
                      sig_sizes, out);
}

void* lb_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void lb_host_free(void* p) {
  if (p) hipHostFree(p);
}

uint32_t lb_pubkey_table_size(const lb_engine* e) { return e ? e->table_n : 0; }
uint32_t lb_pubkey_comb_size(const lb_engine* e) { return e ? e->comb_n : 0; }
uint64_t lb_pubkey_comb_sets(const lb_engine* e) { return e ? e->comb_sets : 0; }
uint64_t lb_subgroup_batch_runs(const lb_engine* e, uint64_t* fallbacks) {
  if (fallbacks) *fallbacks = e ? e->sgb_fallbacks : 0;
  return e ? e->sgb_runs : 0;
}

int32_t lb_pubkey_table_append(lb_engine* e, uint32_t n, const uint8_t* keys, uint32_t key_size, int32_t validate,
                               int32_t* out_status, uint32_t* out_first_index) {
  if (!e || (n && (!keys || !out_status)) || (key_size != 48 && key_size != 96)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  const uint32_t first = e->table_n;
  if (out_first_index) *out_first_index = first;
  if (!n) return LB_OK;
  const uint32_t need = first + n;
  if (need > e->table_cap) {
    // grow: records keep their layout, one contiguous copy
    uint32_t cap = e->table_cap ? e->table_cap : 1024;
    while (cap < need) cap *= 2;
    dbuf nt;
    LB_HIP(nt.ensure((size_t)cap * LB_TABLE_REC * 4));
    if (first)
      LB_HIP(hipMemcpyAsync(nt.p, e->table.p, (size_t)first * LB_TABLE_REC * 4, hipMemcpyDeviceToDevice, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    e->table.release();
    e->table = nt;
    e->table_cap = cap;
  }
  // the comb entries grow with the records, up to the budget's key count
  uint32_t comb_need = std::min(need, e->comb_max);
  if (comb_need > e->comb_cap) {
    const uint32_t cap = std::min(e->table_cap, e->comb_max);
    const size_t rec = (size_t)LB_COMB_ENTRIES * sizeof(g1a);
    dbuf nc;
    hipError_t rc = nc.ensure((size_t)cap * rec);
    if (rc == hipSuccess && e->comb_n)
      rc = hipMemcpyAsync(nc.p, e->comb.p, (size_t)e->comb_n * rec, hipMemcpyDeviceToDevice, e->stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e->stream);
    if (rc == hipSuccess) {
      e->comb.release();
      e->comb = nc;
      e->comb_cap = cap;
    } else {
      // no memory for more entries: the registration still succeeds, the coverage stays where it
      // is (the keys registered from here on take the ladder)
      nc.release();
      (void)hipGetLastError();
      fprintf(stderr, "lodestar_bls: no memory for %u keys' window tables (%s): coverage stays at %u keys\n", cap,
              hipGetErrorString(rc), e->comb_n);
      e->comb_max = e->comb_n;
      comb_need = e->comb_n;
    }
  }
  dbuf kin, st;
  hipError_t r = kin.ensure((size_t)n * key_size);
  if (r == hipSuccess) r = st.ensure((size_t)n * 4);
  if (r == hipSuccess) r = hipMemcpyAsync(kin.p, keys, (size_t)n * key_size, hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(k_table_fill, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n, kin.as<uint8_t>(), key_size,
                       validate, first, e->table.as<uint32_t>(), st.as<int32_t>());
    r = hipGetLastError();
  }
  if (r == hipSuccess && comb_need > first) {  // keys [first, comb_need): inside the budget
    const uint32_t nk = comb_need - first;
    hipLaunchKernelGGL(k_comb_fill, dim3((nk + 7) / 8, LB_COMB_J), dim3(LB_INV_TPB), 0, e->stream, nk, first,
                       e->table.as<uint32_t>(), e->comb.as<uint32_t>());
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(out_status, st.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  kin.release();
  st.release();
  if (r != hipSuccess) {
    fprintf(stderr, "lodestar_bls: pubkey table append failed: %s\n", hipGetErrorString(r));
    return LB_ERR_DEVICE;
  }
  e->table_n = need;
  e->comb_n = std::max(e->comb_n, comb_need);
  return LB_OK;
}

void lb_batch_destroy(lb_batch* b) {
  if (!b) return;
  hipSetDevice(b->device);
  delete b;
}
uint32_t lb_batch_num_sets(const lb_batch* b) { return b ? b->n_sets : 0; }
uint32_t lb_batch_num_jobs(const lb_batch* b) { return b ? b->n_jobs : 0; }

}  // extern "C"

// stage timing helpers (HIP events on the stage's own stream)
struct stage_scope {
  lb_engine* e;
  int k;
  hipStream_t st;
  stage_scope(lb_engine* e_, int k_, hipStream_t st_) : e(e_), k(k_), st(st_) {
    if (e->profiling) {
      hipEventRecord(e->ev0[k], st);
      e->used[k] = true;
    }
  }
  ~stage_scope() {
    if (e->profiling) hipEventRecord(e->ev1[k], st);
  }
};

// Bucket sums -> S_j = sum_d d B_d per instance j (n_inst instances of W windows, buckets
// [j W 256, (j+1) W 256) of bsum) -> element out0 + j of `out` (SoA, stride n_out).
// entries: bucket entries (point, window) of the launch, an upper bound; the forms: pipe_plan_msm.
// ev_bsum (optional): recorded on st after the bucket sums, before their reduction.
static hipError_t msm_reduce(lb_engine* e, hipStream_t st, uint32_t bcap, uint32_t nb, uint32_t n_inst, int W,
                             uint32_t* out, uint32_t n_out, uint32_t out0, uint64_t entries, uint32_t chunk,
                             hipEvent_t ev_bsum = nullptr) {
  const pipe_msm_plan p = pipe_plan_msm(e->knobs, entries, chunk, nb, device_alone(e));
  const bool w4 = W == LB_MSM_W;  // else LB_SMSM_W windows
  if (p.reduce == MSMR_WINDOW_HORNER) {
    hipError_t r = e->wsum.ensure((size_t)n_inst * W * sizeof(g2j));
    if (r != hipSuccess) return r;
  }
  const bool bg8 = p.buckets == MSMB_G8;  // one wave per bucket, else one lane
  hipLaunchKernelGGL(bg8 ? k_msm_buckets_g8 : k_msm_buckets, dim3(bg8 ? nb : nblk(nb)), dim3(bg8 ? 64 : LB_TPB), 0, st,
                     e->bch.as<uint32_t>(), e->bacc.as<uint32_t>(), bcap, e->bsum.as<uint32_t>(), nb);
  if (ev_bsum) {
    const hipError_t r = hipEventRecord(ev_bsum, st);
    if (r != hipSuccess) return r;
  }
  switch (p.reduce) {
    case MSMR_WINDOW_HORNER:
      hipLaunchKernelGGL(k_msm_window_g8, dim3(n_inst * W), dim3(256), 0, st, e->bsum.as<uint32_t>(), nb,
                         e->wsum.as<uint32_t>(), n_inst * W);
      hipLaunchKernelGGL(w4 ? k_msm_horner_g8<LB_MSM_W> : k_msm_horner_g8<LB_SMSM_W>, dim3((n_inst + 7) / 8), dim3(64), 0,
                         st, e->wsum.as<uint32_t>(), n_inst, out, n_out, out0);
      break;
    case MSMR_REDUCE:
      hipLaunchKernelGGL(w4 ? k_msm_reduce<LB_MSM_W> : k_msm_reduce<LB_SMSM_W>, dim3(n_inst), dim3(64 * W), 0, st,
                         e->bsum.as<uint32_t>(), nb, out, n_out, out0);
      break;
  }
  return hipGetLastError();
}

// members per chunk of the per-root sums (the grouping builds the chunks, per_root_chain sums them)
static inline uint32_t gsum_chunk(gsum_form f) { return f == GSUM_WAVE ? LB_GROUP_CHUNK_WAVE : LB_GROUP_CHUNK; }

// s1: P_u = sum of r_i PK_i over the live sets of root u (set_live; k_gsum_*), the Miller loops
// (pipe_plan_miller, with a fresh device_alone sample) into the leaves of the root product tree,
// the tree.  Follows e->plan, the batch plan of the run_pipeline that calls it.
static hipError_t per_root_chain(lb_engine* e, uint32_t n, uint32_t nuh, uint32_t mu) {
  hipStream_t s1 = e->stream;
  const uint32_t* nu = e->n_u.as<uint32_t>();
  const pipe_batch_plan& bp = e->plan;
  {
    stage_scope sc(e, ST_GSUM, s1);
    // chunks of <= gchunk members: at most nuh + n / gchunk of them
    const uint32_t nch = nuh + n / gsum_chunk(bp.gsum);
    switch (bp.gsum) {
      case GSUM_WAVE:
        hipLaunchKernelGGL(k_gsum_wave, dim3(nblk(nch)), dim3(LB_TPB), 0, s1, n, nu, e->gch.as<uint32_t>(),
                           e->chunk_beg.as<uint32_t>(), e->chunk_end.as<uint32_t>(), e->chunk_root.as<uint32_t>(),
                           e->members.as<uint32_t>(), e->set_live.as<uint32_t>(), e->rpk.as<uint32_t>(), e->gacc.as<uint32_t>());
        break;
      case GSUM_CHUNKS:
        hipLaunchKernelGGL(k_gsum_chunks, dim3(nblk(nch)), dim3(LB_TPB), 0, s1, n, nu,
                           e->gch.as<uint32_t>(), e->chunk_beg.as<uint32_t>(), e->chunk_end.as<uint32_t>(),
                           e->members.as<uint32_t>(), e->set_live.as<uint32_t>(), e->rpk.as<uint32_t>(), e->gacc.as<uint32_t>());
        break;
    }
    hipLaunchKernelGGL(k_gsum_final, dim3(nblk_inv(nuh)), dim3(LB_INV_TPB), 0, s1, n, nu, e->gch.as<uint32_t>(),
                       e->gacc.as<uint32_t>(), e->gp_aff.as<uint32_t>(), e->gp_inf.as<uint32_t>(),
                       bp.gsum == GSUM_WAVE ? 1u : 0u);
  }
  {
    stage_scope sc(e, ST_MILLER, s1);
    const miller_form mf = pipe_plan_miller(e->knobs, bp, nuh, device_alone(e));
    switch (mf) {
      case MILLER_ROW:
        hipLaunchKernelGGL(k_miller_row, dim3(nuh), dim3(LBR_NT), 0, s1, n, mu, nu, e->gp_aff.as<uint32_t>(),
                           e->gp_inf.as<uint32_t>(), e->h_aff.as<uint32_t>(), e->treeP.as<uint32_t>());
        break;
      case MILLER_WAVE:
        hipLaunchKernelGGL(k_miller_wave, dim3(nuh), dim3(64), 0, s1, n, mu, nu, e->gp_aff.as<uint32_t>(),
                           e->gp_inf.as<uint32_t>(), e->h_aff.as<uint32_t>(), e->treeP.as<uint32_t>());
        break;
      case MILLER_LANE3:
      case MILLER_LANE2: {
        hipError_t r = e->park.ensure((size_t)2 * 84 * 4 * n);  // T and a temporary per root: two slots of 3 fp2_28
        if (r != hipSuccess) return r;
        hipLaunchKernelGGL(mf == MILLER_LANE3 ? k_miller_lane<3> : k_miller_lane<2>, dim3(nblk(nuh)), dim3(LB_TPB), 0, s1,
                           n, mu, nu, e->gp_aff.as<uint32_t>(), e->gp_inf.as<uint32_t>(), e->h_aff.as<uint32_t>(),
                           e->treeP.as<uint32_t>(), e->park.as<uint32_t>());
        break;
      }
      case MILLER_G8:
        hipLaunchKernelGGL(k_miller_g8, dim3((nuh + LBG_ROOTS - 1) / LBG_ROOTS), dim3(64 * LBG_WAVES), 0, s1, n, mu, nu,
                           e->gp_aff.as<uint32_t>(), e->gp_inf.as<uint32_t>(), e->h_aff.as<uint32_t>(),
                           e->treeP.as<uint32_t>());
        break;
    }
  }
  {
    stage_scope sc(e, ST_TREE_P, s1);
    for (uint32_t lo = mu / 2; lo >= 1; lo /= 2) {
      const bool row = pipe_tree_form(e->knobs, bp, lo) == FE_ROW;
      hipLaunchKernelGGL(row ? k_tree_up_row : k_tree_up_U, dim3(lo), dim3(row ? LBR_NT : 64), 0, s1, mu, lo, nu,
                         e->treeP.as<uint32_t>());
    }
  }
  return hipGetLastError();
}

// Runs the batch pipeline on two streams: the job S tree (leaf count mj = pow2 >= jobs) with
// fS = ML(-G1, S_root) on s2, the message product tree (leaf count mu = pow2 >= sets, leaves
// [0, n_u) live) on s1, joined on s1 ready for the root check.
// force_per_set: the signatures' subgroup check by the per-set kernel whatever the plan says (the
// rerun after a failing per-batch test; e->sgb_active tells the caller which one ran).
static int32_t run_pipeline(lb_engine* e, lb_batch* b, const uint64_t* scalars, uint32_t& mj, uint32_t& mu,
                            bool unblinded, bool force_per_set = false) {
  const uint32_t n = b->n_sets, nj = b->n_jobs;
  e->partial_serial = 0;
  const pipe_shape shape{n, b->n_chunks, b->n_comb, b->indexed, b->route_eng == e, scalars != nullptr, unblinded,
                         e->root_shuffle};
  e->plan = pipe_plan_batch(e->knobs, shape, device_alone(e));
  const pipe_batch_plan& bp = e->plan;
  const bool sgb = n && !force_per_set && pipe_plan_subgroup_batch(bp, shape, e->subgroup_batch);
  e->sgb_active = sgb;
  const uint32_t gchunk = gsum_chunk(bp.gsum);
  int st = fill_scalars(e, n, scalars, unblinded);
  if (st != LB_OK) return st;
  if (sgb) {
    // the tests' bit vectors: fresh per run, from the source of the blinding scalars
    e->h_sgb_bits.resize((size_t)LB_SGB_TESTS * LB_SGB_WORDS);
    size_t need = e->h_sgb_bits.size() * 4, got = 0;
    uint8_t* dst = reinterpret_cast<uint8_t*>(e->h_sgb_bits.data());
    while (got < need) {
      ssize_t r = getrandom(dst + got, need - got, 0);
      if (r < 0) return LB_ERR_DEVICE;
      got += (size_t)r;
    }
    LB_HIP(e->sgb_bits.ensure(need));
    LB_HIP(e->sgb_w.ensure((size_t)LB_SGB_TESTS * sizeof(g2j)));
    LB_HIP(e->sgb_aff.ensure((size_t)LB_SGB_TESTS * sizeof(g2a)));
    LB_HIP(e->sgb_inf.ensure((size_t)LB_SGB_TESTS * 4));
    LB_HIP(e->sgb_status.ensure((size_t)LB_SGB_TESTS * 4));
    LB_HIP(e->sgb_flag.ensure(8));
  }
  mj = 1;
  while (mj < nj) mj <<= 1;
  mu = 1;
  while (mu < n) mu <<= 1;
  const uint32_t mt = mj > mu ? mj : mu;
  const uint32_t ns = n ? n : 1;
  uint32_t cap = 64;
  while (cap < 2 * ns) cap <<= 1;
  LB_HIP(e->scalars.ensure((size_t)ns * 8));
  LB_HIP(e->sig_aff.ensure((size_t)ns * sizeof(g2a)));
  LB_HIP(e->sig_inf.ensure((size_t)ns * 4));
  LB_HIP(e->sig_status.ensure((size_t)ns * 4));
  LB_HIP(e->q.ensure((size_t)ns * 2 * sizeof(g2j)));
  LB_HIP(e->h_aff.ensure((size_t)ns * sizeof(g2a)));
  LB_HIP(e->rpk.ensure((size_t)ns * sizeof(g1j)));
  LB_HIP(e->pk_aff.ensure((size_t)ns * sizeof(g1a)));
  LB_HIP(e->pk_status.ensure((size_t)ns * 4));
  LB_HIP(e->treeP.ensure((size_t)2 * mt * sizeof(fp12)));
  LB_HIP(e->treeS.ensure((size_t)2 * mj * sizeof(g2j)));
  LB_HIP(e->job_status.ensure((size_t)(nj ? nj : 1) * 4));
  LB_HIP(e->fS.ensure(sizeof(fp12)));
  LB_HIP(e->msg_tab.ensure((size_t)cap * 4));
  dbuf* per_set[] = {&e->rep_of, &e->uid_of, &e->uniq_set, &e->set_uid, &e->gcnt, &e->gpos, &e->chunk_beg,
                     &e->chunk_end, &e->members, &e->set_live, &e->gp_inf, &e->chunk_root};
  for (dbuf* d : per_set) LB_HIP(d->ensure((size_t)ns * 4));
  LB_HIP(e->goff.ensure((size_t)(ns + 1) * 4));
  LB_HIP(e->gch.ensure((size_t)(ns + 1) * 4));
  LB_HIP(e->n_u.ensure(4));
  LB_HIP(e->gacc.ensure((size_t)ns * sizeof(g1j)));
  LB_HIP(e->gp_aff.ensure((size_t)ns * sizeof(g1a)));
  const uint32_t bcap = (2 * LB_MSM_W * ns) / LB_MSM_CHUNK + LB_MSM_NB;  // bucket chunks, upper bound
  LB_HIP(e->sig_aos.ensure((size_t)ns * sizeof(g2a)));
  LB_HIP(e->bcnt.ensure((size_t)LB_MSM_NB * 4));
  LB_HIP(e->bcursor.ensure((size_t)LB_MSM_NB * 4));
  LB_HIP(e->boff.ensure((size_t)(LB_MSM_NB + 1) * 4));
  LB_HIP(e->bch.ensure((size_t)(LB_MSM_NB + 1) * 4));
  LB_HIP(e->bchunk_beg.ensure((size_t)bcap * 4));
  LB_HIP(e->bchunk_end.ensure((size_t)bcap * 4));
  LB_HIP(e->bmembers.ensure((size_t)2 * LB_MSM_W * ns * 4));
  LB_HIP(e->bacc.ensure((size_t)bcap * sizeof(g2j)));
  LB_HIP(e->bsum.ensure((size_t)LB_MSM_NB * sizeof(g2j)));
  const uint32_t nc = b->n_chunks;
  LB_HIP(e->chunk_acc.ensure((size_t)(nc ? nc : 1) * sizeof(g1j)));
  LB_HIP(e->chunk_status.ensure((size_t)(nc ? nc : 1) * 4));
  for (int k = 0; k < kStages; k++) {
    e->used[k] = false;
    e->acc_ms[k] = 0.f;
  }
  hipStream_t s1 = e->stream, s2 = e->stream2, s3_ = e->stream3;
  if (e->profiling) {
    hipEventRecord(e->ev0[ST_TOTAL], s1);
    e->used[ST_TOTAL] = true;
  }
  if (n) LB_HIP(hipMemcpyAsync(e->scalars.p, e->h_scalars.data(), (size_t)n * 8, hipMemcpyHostToDevice, s1));
  if (sgb) LB_HIP(hipMemcpyAsync(e->sgb_bits.p, e->h_sgb_bits.data(), e->h_sgb_bits.size() * 4, hipMemcpyHostToDevice, s1));
  // fork: s2 starts after s1's scalar upload
  LB_HIP(hipEventRecord(e->ev_fork, s1));
  LB_HIP(hipStreamWaitEvent(s2, e->ev_fork, 0));
  LB_HIP(hipStreamWaitEvent(s3_, e->ev_fork, 0));
  const uint32_t* nu = e->n_u.as<uint32_t>();
  if (n) {
    // ---- pubkeys, r*PK: on s3 beside the signature decode, or on s2 before it
    const bool pk_split = bp.pk_on == PK_ON_S3;  // on its own stream the pubkey side splits: statuses, then r PK
    const hipStream_t s3 = pk_split ? s3_ : s2;
    // r_i sig_i on s3 beside the subgroup check (small batches alone, row forms, one-workgroup sum)
    const bool sb_par = bp.ssum == SSUM_PAR_W4;
    {
      stage_scope sc(e, ST_PK_CHUNKS, s3);
      switch (bp.pk_chunks) {
        case PKC_INDEXED:
          hipLaunchKernelGGL(k_pk_chunks_idx, dim3(nblk(nc)), dim3(LB_TPB), 0, s3, nc, b->d_chunk_lo.as<uint32_t>(),
                             b->d_pks.as<uint32_t>(), e->table.as<uint32_t>(), e->table_n, e->chunk_acc.as<uint32_t>(),
                             e->chunk_status.as<int32_t>());
          break;
        case PKC_BYTES:
          hipLaunchKernelGGL(k_pk_chunks, dim3(nblk(nc)), dim3(LB_TPB), 0, s3, nc, b->d_chunk_lo.as<uint32_t>(),
                             b->d_pks.as<uint8_t>(), e->chunk_acc.as<uint32_t>(), e->chunk_status.as<int32_t>());
          break;
        case PKC_NONE:
          break;
      }
    }
    {
      stage_scope sc(e, ST_PK_BLIND, s3);
      // k_pk_blind's modes: 0 all; 1 aggregate + status, then 2 the per-set ladder
      const uint32_t mode0 = bp.pk_blind == PKB_ONE_PASS ? 0u : 1u;
      hipLaunchKernelGGL(k_pk_blind, dim3(nblk_inv(n)), dim3(LB_INV_TPB), 0, s3, n, nc, b->d_set_chunk_off.as<uint32_t>(),
                         e->chunk_acc.as<uint32_t>(), e->chunk_status.as<int32_t>(), e->pk_aff.as<uint32_t>(),
                         e->scalars.as<uint64_t>(), e->rpk.as<uint32_t>(), e->pk_status.as<int32_t>(), mode0, nullptr, 0u);
      if (mode0 == 1u) LB_HIP(hipEventRecord(e->ev_pkst, s3));
      switch (bp.pk_blind) {
        case PKB_ONE_PASS:
          break;
        case PKB_SPLIT:
          hipLaunchKernelGGL(k_pk_blind, dim3(nblk_inv(n)), dim3(LB_INV_TPB), 0, s3, n, nc, b->d_set_chunk_off.as<uint32_t>(),
                             e->chunk_acc.as<uint32_t>(), e->chunk_status.as<int32_t>(), e->pk_aff.as<uint32_t>(),
                             e->scalars.as<uint64_t>(), e->rpk.as<uint32_t>(), e->pk_status.as<int32_t>(), 2u, nullptr, 0u);
          break;
        case PKB_SPLIT_ROWP:
          hipLaunchKernelGGL(k_pk_blind_rowp, dim3(n), dim3(64), 0, s3, n, e->pk_aff.as<uint32_t>(),
                             e->scalars.as<uint64_t>(), e->rpk.as<uint32_t>(), e->pk_status.as<int32_t>());
          break;
        case PKB_ROUTE: {
          // the comb over the batch's single-key sets and the ladder over the compacted rest
          const uint32_t n_lad = n - b->n_comb;
          const uint32_t* sel = b->d_route.as<uint32_t>();
          hipLaunchKernelGGL(k_pk_blind_comb, dim3(nblk(b->n_comb)), dim3(LB_TPB), 0, s3, n, b->n_comb, sel,
                             b->d_pk_off.as<uint32_t>(), b->d_pks.as<uint32_t>(), e->comb.as<uint32_t>(), e->comb_n,
                             e->pk_aff.as<uint32_t>(), e->scalars.as<uint64_t>(), e->pk_status.as<int32_t>(),
                             e->rpk.as<uint32_t>());
          e->comb_sets += b->n_comb;
          if (n_lad)
            hipLaunchKernelGGL(k_pk_blind, dim3(nblk_inv(n_lad)), dim3(LB_INV_TPB), 0, s3, n, nc,
                               b->d_set_chunk_off.as<uint32_t>(), e->chunk_acc.as<uint32_t>(), e->chunk_status.as<int32_t>(),
                               e->pk_aff.as<uint32_t>(), e->scalars.as<uint64_t>(), e->rpk.as<uint32_t>(),
                               e->pk_status.as<int32_t>(), 2u, sel + b->n_comb, n_lad);
          break;
        }
      }
    }
    LB_HIP(hipEventRecord(e->ev_pk, s3));
    // signatures: decoded while s1 groups and hashes the messages
    {
      stage_scope sc(e, ST_DECODE, s2);
      const bool drow = bp.decode == DEC_ROW;  // two signatures per wave, else one per lane
      hipLaunchKernelGGL(drow ? k_decompress_sigs_row : k_decompress_sigs, dim3(drow ? (n + 1) / 2 : nblk(n)),
                         dim3(drow ? 64 : LB_TPB), 0, s2, n, b->d_sigs.as<uint8_t>(),
                         b->has_sizes ? b->d_sig_sizes.as<uint32_t>() : nullptr, e->sig_aff.as<uint32_t>(),
                         e->sig_aos.as<uint4>(), e->sig_inf.as<uint32_t>(), e->sig_status.as<int32_t>());
      if (sb_par) LB_HIP(hipEventRecord(e->ev_sdec, s2));
      // (the per-batch test: no per-set kernel; sig_status stays as the decode left it)
      if (!sgb) switch (bp.subgroup) {
        case SUBGROUP_W4:
          hipLaunchKernelGGL(k_sig_subgroup_w4, dim3(n), dim3(64), 0, s2, n, e->sig_aff.as<uint32_t>(),
                             e->sig_inf.as<uint32_t>(), e->sig_status.as<int32_t>());
          break;
        case SUBGROUP_G8:
          hipLaunchKernelGGL(k_sig_subgroup_g8, dim3((n + 7) / 8), dim3(64), 0, s2, n, e->sig_aff.as<uint32_t>(),
                             e->sig_inf.as<uint32_t>(), e->sig_status.as<int32_t>());
          break;
        case SUBGROUP_LANE:
          hipLaunchKernelGGL(k_sig_subgroup, dim3(nblk(n)), dim3(LB_TPB), 0, s2, n, e->sig_aff.as<uint32_t>(),
                             e->sig_inf.as<uint32_t>(), e->sig_status.as<int32_t>());
          break;
      }
      LB_HIP(hipStreamWaitEvent(s2, pk_split ? e->ev_pkst : e->ev_pk, 0));  // job statuses need the pubkey statuses
      hipLaunchKernelGGL(k_job_status, dim3(nblk(nj)), dim3(LB_TPB), 0, s2, nj, b->d_job_off.as<uint32_t>(),
                         e->sig_status.as<int32_t>(), e->pk_status.as<int32_t>(), e->job_status.as<int32_t>(),
                         e->set_live.as<uint32_t>());
    }
    LB_HIP(hipEventRecord(e->ev_dec, s2));
    if (sb_par) {
      // r_i sig_i of every decoded set on s3 (after its pubkey work) beside s2's subgroup check and
      // job statuses; the sum on s2 masks the terms by liveness
      LB_HIP(hipStreamWaitEvent(s3, e->ev_sdec, 0));
      if (e->profiling) {
        hipEventRecord(e->ev0[ST_SIG_MSM], s3);
        e->used[ST_SIG_MSM] = true;
      }
      LB_HIP(e->s_terms.ensure((size_t)n * sizeof(g2j)));
      hipLaunchKernelGGL(k_sig_blind_w4, dim3(n), dim3(64), 0, s3, n, e->sig_aff.as<uint32_t>(),
                         e->scalars.as<uint64_t>(), e->sig_inf.as<uint32_t>(), e->s_terms.as<uint32_t>());
      LB_HIP(hipEventRecord(e->ev_sblind, s3));
    }
    // ---- s1: group the sets by signing root
    {
      stage_scope sc(e, ST_DEDUP, s1);
      if (bp.group == GROUP_ONE_SET) {
        hipLaunchKernelGGL(k_dedup_one, dim3(1), dim3(64), 0, s1, e->rep_of.as<uint32_t>(), e->uid_of.as<uint32_t>(),
                           e->uniq_set.as<uint32_t>(), e->n_u.as<uint32_t>(), e->set_uid.as<uint32_t>(),
                           e->gcnt.as<uint32_t>(), e->gpos.as<uint32_t>(), e->goff.as<uint32_t>(), e->gch.as<uint32_t>(),
                           e->chunk_beg.as<uint32_t>(), e->chunk_end.as<uint32_t>(), e->chunk_root.as<uint32_t>(),
                           e->members.as<uint32_t>());
      } else {
        LB_HIP(hipMemsetAsync(e->msg_tab.p, 0xff, (size_t)cap * 4, s1));
        LB_HIP(hipMemsetAsync(e->n_u.p, 0, 4, s1));
        LB_HIP(hipMemsetAsync(e->gcnt.p, 0, (size_t)n * 4, s1));
        hipLaunchKernelGGL(k_msg_insert, dim3(nblk(n)), dim3(LB_TPB), 0, s1, n, b->d_msgs.as<uint8_t>(), e->msg_key,
                           cap, e->msg_tab.as<uint32_t>(), e->rep_of.as<uint32_t>());
        if (bp.group == GROUP_DEVICE_ORDER)
          hipLaunchKernelGGL(k_msg_uid, dim3(nblk(cap)), dim3(LB_TPB), 0, s1, cap, e->msg_tab.as<uint32_t>(),
                             e->uid_of.as<uint32_t>(), e->uniq_set.as<uint32_t>(), e->n_u.as<uint32_t>());
        else {
          // input order (LB_ROOT_SHUFFLE=0: A/B and the search-trace tests), made deterministic on
          // the host: roots numbered by first occurrence and members in input order within a root
          // (the device form's atomics order both by wave scheduling, so two runs of one batch
          // could build different root trees)
          std::vector<uint32_t> rep(n), uid(n, 0xffffffffu), uniq, suid(n), cnt, pos(n);
          LB_HIP(hipMemcpyAsync(rep.data(), e->rep_of.p, (size_t)n * 4, hipMemcpyDeviceToHost, s1));
          LB_HIP(hipStreamSynchronize(s1));
          for (uint32_t i = 0; i < n; i++) {
            const uint32_t r = rep[i];
            if (uid[r] == 0xffffffffu) {
              uid[r] = (uint32_t)uniq.size();
              uniq.push_back(r);
              cnt.push_back(0);
            }
            suid[i] = uid[r];
            pos[i] = cnt[uid[r]]++;
          }
          const uint32_t nun = (uint32_t)uniq.size();
          LB_HIP(hipMemcpyAsync(e->uid_of.p, uid.data(), (size_t)n * 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipMemcpyAsync(e->uniq_set.p, uniq.data(), (size_t)nun * 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipMemcpyAsync(e->set_uid.p, suid.data(), (size_t)n * 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipMemcpyAsync(e->gcnt.p, cnt.data(), (size_t)nun * 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipMemcpyAsync(e->gpos.p, pos.data(), (size_t)n * 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipMemcpyAsync(e->n_u.p, &nun, 4, hipMemcpyHostToDevice, s1));
          LB_HIP(hipStreamSynchronize(s1));
        }
        if (bp.group == GROUP_DEVICE_ORDER)
          hipLaunchKernelGGL(k_msg_count, dim3(nblk(n)), dim3(LB_TPB), 0, s1, n, e->rep_of.as<uint32_t>(),
                             e->uid_of.as<uint32_t>(), e->set_uid.as<uint32_t>(), e->gcnt.as<uint32_t>(),
                             e->gpos.as<uint32_t>());
        hipLaunchKernelGGL(k_msg_scan, dim3(1), dim3(1024), 0, s1, nu, 0u, gchunk, e->gcnt.as<uint32_t>(), e->goff.as<uint32_t>(),
                           e->gch.as<uint32_t>(), nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(k_chunk_fill, dim3(nblk(n + n / gchunk + 1)), dim3(LB_TPB), 0, s1, nu,
                           gchunk, e->goff.as<uint32_t>(), e->gch.as<uint32_t>(),
                           e->chunk_beg.as<uint32_t>(), e->chunk_end.as<uint32_t>(), e->chunk_root.as<uint32_t>());
        hipLaunchKernelGGL(k_msg_scatter, dim3(nblk(n)), dim3(LB_TPB), 0, s1, n, e->set_uid.as<uint32_t>(),
                           e->gpos.as<uint32_t>(), e->goff.as<uint32_t>(), e->members.as<uint32_t>());
      }
      // distinct-root count to the host: the per-root kernels below are launched over it (a
      // launch over the set count would size their private-segment scratch for n lanes)
      // (one set: one root, known without the round trip)
      if (bp.group == GROUP_ONE_SET) {
        *e->h_nu = 1;
      } else {
        LB_HIP(hipMemcpyAsync(e->h_nu, e->n_u.p, 4, hipMemcpyDeviceToHost, s1));
        LB_HIP(hipStreamSynchronize(s1));
      }
    }
    const uint32_t nuh = *e->h_nu;
    if (nuh == 0 || nuh > n) return LB_ERR_DEVICE;
    const pipe_hash_plan hp = pipe_plan_hash(e->knobs, bp, nuh, device_alone(e));
    mu = 1;
    while (mu < nuh) mu <<= 1;
    // ---- s1: hash_to_G2 once per distinct root
    {
      stage_scope sc(e, ST_HASH_MAP, s1);
      const bool hrow = hp.map == HMAP_ROW;  // one wave per field element, else one lane
      hipLaunchKernelGGL(hrow ? k_hash_map_row : k_hash_map, dim3(hrow ? 2 * nuh : nblk(2 * nuh)), dim3(hrow ? 64 : LB_TPB),
                         0, s1, n, nuh, e->uniq_set.as<uint32_t>(), b->d_msgs.as<uint8_t>(), e->q.as<uint32_t>());
    }
    {
      stage_scope sc(e, ST_HASH_FIN, s1);
      switch (hp.fin) {
        case HFIN_ROW:
          hipLaunchKernelGGL(k_hash_finish_row, dim3(nuh), dim3(LBR_NT), 0, s1, n, nu, e->q.as<uint32_t>(),
                             e->h_aff.as<uint32_t>(), e->hash_row_careful ? 1u : 0u);
          break;
        case HFIN_G8:
          hipLaunchKernelGGL(k_hash_finish_g8, dim3((nuh + 7) / 8), dim3(64), 0, s1, n, nu, e->q.as<uint32_t>(),
                             e->h_aff.as<uint32_t>());
          break;
        case HFIN_LANE: {
          const uint32_t pn = nblk_inv(nuh) * LB_INV_TPB;  // one park column per launched lane
          LB_HIP(e->park.ensure((size_t)4 * 72 * 4 * (pn > n ? pn : n)));
          hipLaunchKernelGGL(k_hash_finish, dim3(nblk_inv(nuh)), dim3(LB_INV_TPB), 0, s1, n, nu, e->q.as<uint32_t>(),
                             e->h_aff.as<uint32_t>(), e->park.as<uint32_t>(), pn);
          break;
        }
      }
    }
    // ---- s2: S = sum r_i sig_i, overlapped with the Miller loops
    switch (bp.ssum) {
      case SSUM_PAR_W4:  // the terms are on their way on s3 (above)
        LB_HIP(hipStreamWaitEvent(s2, e->ev_sblind, 0));
        hipLaunchKernelGGL(k_g2_sum_g8, dim3(1), dim3(8 * LB_SUM_G8_GROUPS), 0, s2, n, e->s_terms.as<uint32_t>(),
                           2 * mj, e->treeS.as<uint32_t>(), 1u, e->set_live.as<uint32_t>());
        if (e->profiling) hipEventRecord(e->ev1[ST_SIG_MSM], s2);
        break;
      case SSUM_UNBLINDED: {
        stage_scope sc(e, ST_SIG_MSM, s2);
        hipLaunchKernelGGL(k_sig_unblinded, dim3(1), dim3(64), 0, s2, e->sig_aff.as<uint32_t>(),
                           e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(), 2 * mj, e->treeS.as<uint32_t>());
        break;
      }
      case SSUM_TERMS_G8:
      case SSUM_TERMS_LANE: {
        stage_scope sc(e, ST_SIG_MSM, s2);
        LB_HIP(e->s_terms.ensure((size_t)n * sizeof(g2j)));
        LB_HIP(e->s_part.ensure((size_t)((n + 63) / 64) * sizeof(g2j)));
        if (bp.ssum == SSUM_TERMS_G8) {  // 8 lanes per set, then one workgroup of 8-lane additions
          hipLaunchKernelGGL(k_sig_blind_g8, dim3((n + 7) / 8), dim3(64), 0, s2, n, e->sig_aff.as<uint32_t>(),
                             e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(),
                             e->s_terms.as<uint32_t>());
          hipLaunchKernelGGL(k_g2_sum_g8, dim3(1), dim3(8 * LB_SUM_G8_GROUPS), 0, s2, n, e->s_terms.as<uint32_t>(),
                             2 * mj, e->treeS.as<uint32_t>(), 1u, nullptr);
          break;
        }
        hipLaunchKernelGGL(k_sig_blind, dim3(nblk_inv(n)), dim3(LB_INV_TPB), 0, s2, n, e->sig_aff.as<uint32_t>(),
                           e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(),
                           e->s_terms.as<uint32_t>());
        // 64:1 levels, ping-ponging between the two buffers; the last level writes treeS[1]
        uint32_t* bufs[2] = {e->s_terms.as<uint32_t>(), e->s_part.as<uint32_t>()};
        uint32_t m = n;
        int cur = 0;
        while (m > 64) {
          const uint32_t mo = (m + 63) / 64;
          hipLaunchKernelGGL(k_g2_sum64, dim3(mo), dim3(64), 0, s2, m, bufs[cur], mo, bufs[cur ^ 1], 0u);
          m = mo;
          cur ^= 1;
        }
        hipLaunchKernelGGL(k_g2_sum64, dim3(1), dim3(64), 0, s2, m, bufs[cur], 2 * mj, e->treeS.as<uint32_t>(), 1u);
        break;
      }
      case SSUM_BUCKET_MSM: {
        stage_scope sc(e, ST_SIG_MSM, s2);
        LB_HIP(hipMemsetAsync(e->bcnt.p, 0, (size_t)LB_MSM_NB * 4, s2));
        LB_HIP(hipMemsetAsync(e->bcursor.p, 0, (size_t)LB_MSM_NB * 4, s2));
        hipLaunchKernelGGL(k_msm_count, dim3(nblk(n)), dim3(LB_TPB), 0, s2, n, e->scalars.as<uint64_t>(),
                           e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(), e->bcnt.as<uint32_t>());
        hipLaunchKernelGGL(k_msg_scan, dim3(1), dim3(1024), 0, s2, nullptr, (uint32_t)LB_MSM_NB, (uint32_t)LB_MSM_CHUNK,
                           e->bcnt.as<uint32_t>(),
                           e->boff.as<uint32_t>(), e->bch.as<uint32_t>(), e->bchunk_beg.as<uint32_t>(),
                           e->bchunk_end.as<uint32_t>(), nullptr);
        hipLaunchKernelGGL(k_msm_scatter, dim3(nblk(n)), dim3(LB_TPB), 0, s2, n, e->scalars.as<uint64_t>(),
                           e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(), e->boff.as<uint32_t>(),
                           e->bcursor.as<uint32_t>(), e->bmembers.as<uint32_t>());
        hipLaunchKernelGGL(k_msm_chunks, dim3(nblk(bcap)), dim3(LB_TPB), 0, s2, e->bch.as<uint32_t>(),
                           e->bchunk_beg.as<uint32_t>(), e->bchunk_end.as<uint32_t>(), e->bmembers.as<uint32_t>(),
                           e->sig_aos.as<uint4>(), bcap, e->bacc.as<uint32_t>(), (uint32_t)LB_MSM_NB);
        LB_HIP(msm_reduce(e, s2, bcap, LB_MSM_NB, 1u, LB_MSM_W, e->treeS.as<uint32_t>(), 2 * mj, 1u,
                          (uint64_t)2 * LB_MSM_W * n, LB_MSM_CHUNK, sgb ? e->ev_bsum : nullptr));
        if (sgb) {
          // the per-batch subgroup test on s3 (idle: a bucket-MSM batch has its pubkey work on s2),
          // beside the bucket reduction and ML(-G1, S), which do not need its result
          LB_HIP(hipStreamWaitEvent(s3_, e->ev_bsum, 0));
          LB_HIP(hipMemsetAsync(e->sgb_flag.p, 0, 8, s3_));
          hipLaunchKernelGGL(k_subgroup_mix, dim3(LB_SGB_TESTS), dim3(64), 0, s3_, e->bsum.as<uint32_t>(),
                             (uint32_t)LB_MSM_NB, e->sgb_bits.as<uint32_t>(), e->sgb_w.as<uint32_t>());
          hipLaunchKernelGGL(k_subgroup_affine, dim3(1), dim3(LB_INV_TPB), 0, s3_, (uint32_t)LB_SGB_TESTS,
                             e->sgb_w.as<uint32_t>(), e->sgb_aff.as<uint32_t>(), e->sgb_inf.as<uint32_t>(),
                             e->sgb_status.as<int32_t>());
          hipLaunchKernelGGL(k_sig_subgroup_g8, dim3(LB_SGB_TESTS / 8), dim3(64), 0, s3_, (uint32_t)LB_SGB_TESTS,
                             e->sgb_aff.as<uint32_t>(), e->sgb_inf.as<uint32_t>(), e->sgb_status.as<int32_t>());
          hipLaunchKernelGGL(k_subgroup_flag, dim3(nblk(std::max<uint32_t>(nj, LB_SGB_TESTS))), dim3(LB_TPB), 0, s3_, nj,
                             b->d_job_off.as<uint32_t>(), e->sig_status.as<int32_t>(), e->sig_inf.as<uint32_t>(),
                             e->pk_status.as<int32_t>(), e->job_status.as<int32_t>(), e->sgb_status.as<int32_t>(),
                             e->sgb_flag.as<uint32_t>());
          LB_HIP(hipEventRecord(e->ev_sgb, s3_));  // (s1 joins it below, after its own chain)
        }
        break;
      }
    }
    // ---- s1: per-root sums of r_i PK_i and the Miller loops, after the signature decode
    LB_HIP(hipStreamWaitEvent(s1, e->ev_dec, 0));
    LB_HIP(hipStreamWaitEvent(s1, e->ev_pk, 0));  // r PK (the decode's wait covered the statuses only)
    LB_HIP(per_root_chain(e, n, nuh, mu));
  } else {
    // no sets: every job is empty; the message tree is the single identity leaf
    LB_HIP(hipEventRecord(e->ev_dec, s2));
    hipLaunchKernelGGL(k_job_status, dim3(nblk(nj)), dim3(LB_TPB), 0, s1, nj, b->d_job_off.as<uint32_t>(),
                       e->sig_status.as<int32_t>(), e->pk_status.as<int32_t>(), e->job_status.as<int32_t>(),
                       e->set_live.as<uint32_t>());
    hipLaunchKernelGGL(k_set_one, dim3(1), dim3(64), 0, s1, e->treeP.as<uint32_t>(), 2 * mu, mu);
  }
  if (!n) {
    // no sets: S_root = infinity
    hipLaunchKernelGGL(k_g2_set_inf, dim3(1), dim3(64), 0, s2, e->treeS.as<uint32_t>(), 2 * mj, 1u);
  }
  // ---- s2: ML(-G1, S_root)
  {
    stage_scope sc(e, ST_ML_S, s2);
    hipLaunchKernelGGL(bp.fe == FE_ROW ? k_ml_S_row : k_ml_S, dim3(1), dim3(bp.fe == FE_ROW ? LBR_NT : 64), 0, s2, mj,
                       e->treeS.as<uint32_t>(), e->fS.as<uint32_t>());
  }
  LB_HIP(hipEventRecord(e->ev_s, s2));
  LB_HIP(hipStreamWaitEvent(s1, e->ev_s, 0));  // join
  if (sgb) LB_HIP(hipStreamWaitEvent(s1, e->ev_sgb, 0));  // the flag words come back with the verdict
  LB_HIP(hipGetLastError());
  return LB_OK;
}

// After the readback that ends a run: counts a run of the per-batch subgroup test and tells whether
// it failed (flag: k_subgroup_flag's two words), i.e. whether the batch runs again by the per-set test.
static bool sgb_failed(lb_engine* e, const uint32_t flag[2]) {
  if (!e->sgb_active) return false;
  e->sgb_runs++;
  if (!(flag[0] | flag[1])) return false;
  e->sgb_fallbacks++;
  return true;
}

// ---------------------------------------------------------------- invalid-set search
// After a failing root check: find the failing SETS (a job fails iff one of its live sets does;
// per-job verdicts then equal the reference's per-job re-verification, worker.ts:76-98, up to
// the 2^-64 soundness of the blinding).  What a round launches and what its results mean is
// device-free code in lb_search_plan.h (the nodes, the two moves, the planner and the
// interpreter); here are the device's part of a launch set (search_round), the per-root sums
// (search_root_sums) and the loop over rounds (search_invalid).  Costs: a few waves and range
// MSMs over the failing ranges per round; about four rounds for a batch of ~10^5 sets with a
// handful of invalid ones.
static_assert(SX_COUNT <= 32, "lb_engine::sx");
static_assert(kWtParts == LB_WT_MAX, "lb_search_plan.h kWtParts");

template <class T>
static hipError_t sx_up(lb_engine* e, int k, const std::vector<T>& v, hipStream_t s) {
  hipError_t r = e->sx[k].ensure((v.empty() ? 1 : v.size()) * sizeof(T));
  if (r == hipSuccess && !v.empty()) r = hipMemcpyAsync(e->sx[k].p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
  return r;
}

// stages run once per search round: their elapsed times join acc_ms (after the round's synchronisation)
static void stage_accumulate(lb_engine* e, std::initializer_list<int> stages) {
  if (!e->profiling) return;
  for (int k : stages) {
    float ms = 0.f;
    if (e->used[k] && hipEventElapsedTime(&ms, e->ev0[k], e->ev1[k]) == hipSuccess) e->acc_ms[k] += ms;
    e->used[k] = false;
  }
}

// the bucket MSM's count (scatter = false) or scatter pass over the round's T positions, W windows
template <int W>
static void smsm_pass(lb_engine* e, hipStream_t s, bool scatter, uint32_t T, uint32_t cm, const smsm_args& ma) {
  if (!scatter)
    hipLaunchKernelGGL(k_smsm_count<W>, dim3(nblk(T)), dim3(LB_TPB), 0, s, T, cm, ma, e->members.as<uint32_t>(),
                       e->set_uid.as<uint32_t>(), e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(),
                       e->sig_inf.as<uint32_t>(), e->bcnt.as<uint32_t>());
  else
    hipLaunchKernelGGL(k_smsm_scatter<W>, dim3(nblk(T)), dim3(LB_TPB), 0, s, T, cm, ma, e->members.as<uint32_t>(),
                       e->set_uid.as<uint32_t>(), e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(),
                       e->sig_inf.as<uint32_t>(), e->boff.as<uint32_t>(), e->bcursor.as<uint32_t>(),
                       e->bmembers.as<uint32_t>());
}

// One launch set on the device: the columns of `tab` up, the range sums S of its MSM instances,
// the direct checks, then the weighted tests (fresh ones first).  Outputs the direct verdicts and
// FE values (144 words each) and each test's matched child (1-based, 0: none).
static int32_t search_round(lb_engine* e, const search_ctx& x, const launch_set& ls, const search_tab& tab,
                            std::vector<int32_t>& verdict, std::vector<uint32_t>& ydir, std::vector<int32_t>& tout) {
  hipStream_t s1 = e->stream;
  const uint32_t c = (uint32_t)ls.D.size(), nt = (uint32_t)ls.tests.size(), n_fresh = ls.n_fresh, n = x.n;
  const bool rs_path = tab.rs_path, w4 = tab.w4;
  const uint32_t nwin = w4 ? (uint32_t)LB_MSM_W : (uint32_t)LB_SMSM_W;
  const uint32_t cm = tab.cm, T = tab.T, nb = cm * nwin * LB_MSM_B;
  const uint32_t schunk = e->search_chunk;
  const uint32_t bcap = (2 * nwin * T) / schunk + nb;
  for (int k : kSxUploads) LB_HIP(sx_up(e, k, tab.col[k], s1));
  const uint32_t N = c + nt;
  LB_HIP(e->sx[SX_VERDICT].ensure((c ? c : 1) * 4));
  LB_HIP(e->sx[SX_Y].ensure((size_t)(N ? N : 1) * 576));
  LB_HIP(e->sx[SX_ML].ensure((size_t)(N ? N : 1) * 2 * 576));
  LB_HIP(e->sx[SX_PK].ensure((c ? c : 1) * sizeof(g1j)));
  LB_HIP(e->sx[SX_S].ensure((cm ? cm : 1) * sizeof(g2j)));
  LB_HIP(e->sx[SX_TOUT].ensure((nt ? nt : 1) * 4));
  LB_HIP(e->sx[SX_TPK].ensure((nt ? nt : 1) * sizeof(g1j)));
  auto U = [&](int k) { return e->sx[k].as<uint32_t>(); };
  {
    stage_scope sc(e, ST_FALLBACK, s1);
    const smsm_args ma{U(SX_MPRE), U(SX_MLO), U(SX_MMODE), U(SX_MWA), U(SX_MWB)};
    const pipe_search_plan sp = pipe_plan_search_round(e->knobs, cm, T, rs_path, device_alone(e));
    if (sp.sums == SRCH_TERMS) {
      // small or root-level round: per-position terms + per-instance segmented sums (no bucket MSM)
      std::vector<uint32_t> blo, bhi, bo;
      blocks64(tab.col[SX_MPRE].data(), cm, blo, bhi, bo);
      const uint32_t nbk = (uint32_t)blo.size();
      LB_HIP(sx_up(e, SX_BLO, blo, s1));
      LB_HIP(sx_up(e, SX_BHI, bhi, s1));
      LB_HIP(sx_up(e, SX_BO, bo, s1));
      LB_HIP(e->s_terms.ensure((size_t)T * sizeof(g2j)));
      LB_HIP(e->s_part.ensure((size_t)(nbk ? nbk : 1) * sizeof(g2j)));
      switch (sp.terms) {
        case STERMS_ROOT_SUMS:
          hipLaunchKernelGGL(k_rsm_terms, dim3(nblk(T)), dim3(LB_TPB), 0, s1, T, cm, ma, e->s_root.as<uint32_t>(), x.nu,
                             e->s_terms.as<uint32_t>());
          break;
        case STERMS_LANE:
          hipLaunchKernelGGL(k_smsm_terms_lane, dim3(nblk_inv(T)), dim3(LB_INV_TPB), 0, s1, T, cm, ma,
                             e->members.as<uint32_t>(), e->set_uid.as<uint32_t>(), e->scalars.as<uint64_t>(),
                             e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(), e->sig_aff.as<uint32_t>(), n,
                             e->s_terms.as<uint32_t>());
          break;
        case STERMS_G8:
          hipLaunchKernelGGL(k_smsm_terms_g8, dim3((T + 7) / 8), dim3(64), 0, s1, T, cm, ma, e->members.as<uint32_t>(),
                             e->set_uid.as<uint32_t>(), e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(),
                             e->sig_inf.as<uint32_t>(), e->sig_aff.as<uint32_t>(), n, e->s_terms.as<uint32_t>());
          break;
      }
      if (nbk)
        hipLaunchKernelGGL(k_seg_sum64, dim3(nbk), dim3(64), 0, s1, U(SX_BLO), U(SX_BHI), T, e->s_terms.as<uint32_t>(),
                           nbk, e->s_part.as<uint32_t>(), nullptr);
      hipLaunchKernelGGL(k_seg_final, dim3(cm), dim3(64), 0, s1, U(SX_BO), e->s_part.as<uint32_t>(), nbk ? nbk : 1u,
                         U(SX_S), cm);
    } else if (sp.sums == SRCH_BUCKET_MSM) {
      LB_HIP(e->bcnt.ensure((size_t)nb * 4));
      LB_HIP(e->bcursor.ensure((size_t)nb * 4));
      LB_HIP(e->boff.ensure((size_t)(nb + 1) * 4));
      LB_HIP(e->bch.ensure((size_t)(nb + 1) * 4));
      LB_HIP(e->bchunk_beg.ensure((size_t)bcap * 4));
      LB_HIP(e->bchunk_end.ensure((size_t)bcap * 4));
      LB_HIP(e->bmembers.ensure((size_t)2 * nwin * (T ? T : 1) * 4));
      LB_HIP(e->bacc.ensure((size_t)bcap * sizeof(g2j)));
      LB_HIP(e->bsum.ensure((size_t)nb * sizeof(g2j)));
      LB_HIP(hipMemsetAsync(e->bcnt.p, 0, (size_t)nb * 4, s1));
      LB_HIP(hipMemsetAsync(e->bcursor.p, 0, (size_t)nb * 4, s1));
      const auto pass = w4 ? smsm_pass<LB_MSM_W> : smsm_pass<LB_SMSM_W>;
      if (T) pass(e, s1, false, T, cm, ma);
      hipLaunchKernelGGL(k_msg_scan, dim3(1), dim3(1024), 0, s1, nullptr, nb, schunk, e->bcnt.as<uint32_t>(),
                         e->boff.as<uint32_t>(), e->bch.as<uint32_t>(), e->bchunk_beg.as<uint32_t>(),
                         e->bchunk_end.as<uint32_t>(), nullptr);
      if (T) pass(e, s1, true, T, cm, ma);
      hipLaunchKernelGGL(k_msm_chunks, dim3(nblk(bcap)), dim3(LB_TPB), 0, s1, e->bch.as<uint32_t>(),
                         e->bchunk_beg.as<uint32_t>(), e->bchunk_end.as<uint32_t>(), e->bmembers.as<uint32_t>(),
                         e->sig_aos.as<uint4>(), bcap, e->bacc.as<uint32_t>(), nb);
      LB_HIP(msm_reduce(e, s1, bcap, nb, cm, w4 ? LB_MSM_W : LB_SMSM_W, U(SX_S), cm, 0u, (uint64_t)2 * nwin * T,
                        schunk));
    }
    if (c)
      hipLaunchKernelGGL(k_range_pk, dim3(nblk(c)), dim3(LB_TPB), 0, s1, c, U(SX_KIND), U(SX_LO), U(SX_LEN),
                         e->members.as<uint32_t>(), e->set_live.as<uint32_t>(), n, e->rpk.as<uint32_t>(), U(SX_PK));
    if (nt)
      hipLaunchKernelGGL(k_test_pk, dim3(nt), dim3(64), 0, s1, nt, U(SX_TMODE), U(SX_TLO), U(SX_TLEN), U(SX_TPER),
                         e->members.as<uint32_t>(), e->set_live.as<uint32_t>(), n, e->rpk.as<uint32_t>(), U(SX_TPK));
  }
  {
    stage_scope sc(e, ST_BISECT, s1);
    const srch_items I{c, nt, n_fresh, e->search_merge ? 0u : 1u, U(SX_KIND), U(SX_KEY), U(SX_MIDX), U(SX_TMODE), U(SX_TF), U(SX_TV0),
                       U(SX_TU), U(SX_TMIDX), U(SX_TYIDX)};
    auto stage = [&](uint32_t it0, uint32_t cnt) {
      if (!cnt) return;
      hipLaunchKernelGGL(k_search_ml, dim3(2 * cnt), dim3(64), 0, s1, I, it0, cnt, cm ? cm : 1u, e->treeP.as<uint32_t>(),
                         2 * x.mu, U(SX_PK), U(SX_TPK), e->h_aff.as<uint32_t>(), n, U(SX_S), e->pk_aff.as<uint32_t>(),
                         e->sig_aff.as<uint32_t>(), e->sig_inf.as<uint32_t>(), e->set_live.as<uint32_t>(),
                         e->set_uid.as<uint32_t>(), U(SX_Y), U(SX_ML));
      hipLaunchKernelGGL(k_search_fe, dim3(cnt), dim3(64), 0, s1, I, it0, cnt, U(SX_ML), U(SX_Y),
                         e->sx[SX_VERDICT].as<int32_t>());
    };
    if (e->search_merge) {
      stage(0, c + nt);
    } else {
      stage(0, c + n_fresh);             // direct checks and fresh tests
      stage(c + n_fresh, nt - n_fresh);  // look-ahead tests of the failing direct checks
    }
    if (nt) hipLaunchKernelGGL(k_search_match, dim3(nt), dim3(64), 0, s1, I, U(SX_YUP), U(SX_Y), e->sx[SX_TOUT].as<int32_t>());
  }
  LB_HIP(hipGetLastError());
  verdict.resize(c);
  ydir.resize((size_t)144 * N);  // SoA, stride N = c + nt (direct checks first)
  tout.resize(nt);
  if (c) {
    LB_HIP(hipMemcpyAsync(verdict.data(), e->sx[SX_VERDICT].p, (size_t)c * 4, hipMemcpyDeviceToHost, s1));
    LB_HIP(hipMemcpyAsync(ydir.data(), e->sx[SX_Y].p, (size_t)N * 576, hipMemcpyDeviceToHost, s1));
  }
  if (nt) LB_HIP(hipMemcpyAsync(tout.data(), e->sx[SX_TOUT].p, (size_t)nt * 4, hipMemcpyDeviceToHost, s1));
  LB_HIP(hipStreamSynchronize(s1));
  stage_accumulate(e, {ST_FALLBACK, ST_BISECT});
  return LB_OK;
}

// S_u = sum r_i sig_i over the live sets of each root u (members order): the per-set terms one
// lane per set (k_sig_blind), then segmented sums over each root's positions (blocks of <= 64 of
// one root, then one wave per root).  Once per search, for large batches: the root-level
// instances of a round (subtrees and weighted subtree tests) then cost a 7-bit multiple per ROOT.
static int32_t search_root_sums(lb_engine* e, const search_ctx& x) {
  hipStream_t s1 = e->stream;
  const uint32_t n = x.n, nu = x.nu;
  std::vector<uint32_t> idx, bhi, bo;  // idx: blo[nbk] | bhi[nbk] | bo[nu + 1]
  blocks64(x.goff.data(), nu, idx, bhi, bo);
  const uint32_t nbk = (uint32_t)idx.size();
  idx.insert(idx.end(), bhi.begin(), bhi.end());
  idx.insert(idx.end(), bo.begin(), bo.end());
  LB_HIP(e->rs_idx.ensure(idx.size() * 4));
  LB_HIP(e->s_set.ensure((size_t)n * sizeof(g2j)));
  LB_HIP(e->s_part.ensure((size_t)(nbk ? nbk : 1) * sizeof(g2j)));
  LB_HIP(e->s_root.ensure((size_t)nu * sizeof(g2j)));
  LB_HIP(hipMemcpyAsync(e->rs_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s1));
  const uint32_t* d_idx = e->rs_idx.as<uint32_t>();
  {
    stage_scope sc(e, ST_FALLBACK, s1);
    hipLaunchKernelGGL(k_sig_blind, dim3(nblk_inv(n)), dim3(LB_INV_TPB), 0, s1, n, e->sig_aff.as<uint32_t>(),
                       e->scalars.as<uint64_t>(), e->set_live.as<uint32_t>(), e->sig_inf.as<uint32_t>(),
                       e->s_set.as<uint32_t>());
    if (nbk)
      hipLaunchKernelGGL(k_seg_sum64, dim3(nbk), dim3(64), 0, s1, d_idx, d_idx + nbk, n, e->s_set.as<uint32_t>(), nbk,
                         e->s_part.as<uint32_t>(), e->members.as<uint32_t>());
    hipLaunchKernelGGL(k_seg_final, dim3(nu), dim3(64), 0, s1, d_idx + 2 * nbk, e->s_part.as<uint32_t>(),
                       nbk ? nbk : 1u, e->s_root.as<uint32_t>(), nu);
  }
  LB_HIP(hipGetLastError());
  LB_HIP(hipStreamSynchronize(s1));
  stage_accumulate(e, {ST_FALLBACK});
  return LB_OK;
}

static int32_t search_invalid(lb_engine* e, lb_batch* b, uint32_t mu, int32_t* out_job) {
  const uint32_t n = b->n_sets;
  search_ctx x;
  x.n = n;
  x.mu = mu;
  x.L = 0;
  while ((1u << x.L) < mu) x.L++;
  x.nu = *e->h_nu;
  x.goff.resize(x.nu + 1);
  x.members.resize(n);
  fnode root{{0u, 1u, 0u, n, 0u}, true, std::vector<uint32_t>(144)};
  LB_HIP(hipMemcpyAsync(x.goff.data(), e->goff.p, (size_t)(x.nu + 1) * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(x.members.data(), e->members.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(root.y.data(), e->y_root.p, 576, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  // the first round's form for large batches (see lb_engine::search_blk)
  const pipe_search_start ss = pipe_plan_search_start(e->knobs, e->search_blk, e->search_rootsum, n, x.nu);
  const bool r1_plain = ss.r1_plain;
  if (ss.root_sums) {
    const int32_t st = search_root_sums(e, x);
    if (st != LB_OK) return st;
    x.rs = true;
  }
  std::vector<fnode> F{root}, work;
  std::vector<uint32_t> bad_pos;
  const bool trace = std::getenv("LB_SEARCH_TRACE") != nullptr;
  for (int round = 1; !F.empty(); round++) {
    std::vector<fnode> next;
    search_settle(x, round, F, work, bad_pos);
    const bool spec_on = device_alone(e);
    for (size_t a = 0; a < work.size();) {
      const launch_set ls = search_launch_set(x, work, a, spec_on, r1_plain, round);
      std::vector<int32_t> verdict, tout;
      std::vector<uint32_t> ydir;
      const auto t0 = std::chrono::steady_clock::now();
      const search_tab tab = search_tables(x, ls.Fs, ls.D, ls.tests, ls.n_fresh, e->knobs.search_small_max);
      const int32_t st = search_round(e, x, ls, tab, verdict, ydir, tout);
      if (st != LB_OK) return st;
      if (trace)
        std::fprintf(stderr, "[lb search] round %d: %zu failing nodes, %zu direct checks, %zu weighted tests: %.3f ms\n",
                     round, ls.Fs.size(), ls.D.size(), ls.tests.size(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      search_interpret(ls, verdict, ydir, tout, next, bad_pos);
    }
    F.swap(next);
  }
  search_jobs(x, bad_pos, b->job_off, b->n_jobs, out_job);
  return LB_OK;
}

static void finish_profile(lb_engine* e) {
  if (!e->profiling) return;
  hipStreamSynchronize(e->stream3);
  hipStreamSynchronize(e->stream2);
  hipStreamSynchronize(e->stream);
  for (int k = 0; k < kStages; k++) {
    float ms = 0.f;
    if (e->used[k]) hipEventElapsedTime(&ms, e->ev0[k], e->ev1[k]);
    e->last_ms[k] = ms + e->acc_ms[k];
  }
}

// caller holds e->mu
static int32_t verify_locked(lb_engine* e, lb_batch* b, const uint64_t* scalars, int32_t* out_job) {
  LB_HIP(hipSetDevice(e->device));
  const uint32_t nj = b->n_jobs;
  if (nj == 0) return LB_OK;
  uint32_t m = 1, mu = 1;
  busy_scope busy(e->device, e, e->latency);
  int32_t st;
  std::vector<int32_t> jst(nj);
  int32_t root_ok = 0;
  // a failing per-batch subgroup test discards its run, before any search round: the batch runs
  // again by the per-set test, which is what gives the codes
  for (bool per_set = false;; per_set = true) {
    st = run_pipeline(e, b, scalars, m, mu, true, per_set);
    if (st != LB_OK) return st;
    // root verdict on s1 (after the join)
    LB_HIP(e->verdict.ensure(4));
    {
      stage_scope sc(e, ST_ROOT, e->stream);
      LB_HIP(e->y_root.ensure(576));
      hipLaunchKernelGGL(e->plan.fe == FE_ROW ? k_root_check_row : k_root_check, dim3(1), dim3(e->plan.fe == FE_ROW ? LBR_NT : 64), 0, e->stream, mu, e->treeP.as<uint32_t>(),
                         e->fS.as<uint32_t>(), e->verdict.as<int32_t>(), e->y_root.as<uint32_t>());
    }
    LB_HIP(hipGetLastError());
    uint32_t sgb_flag[2] = {0u, 0u};
    LB_HIP(hipMemcpyAsync(jst.data(), e->job_status.p, (size_t)nj * 4, hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipMemcpyAsync(&root_ok, e->verdict.p, 4, hipMemcpyDeviceToHost, e->stream));
    if (e->sgb_active) LB_HIP(hipMemcpyAsync(sgb_flag, e->sgb_flag.p, 8, hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    if (!sgb_failed(e, sgb_flag)) break;
  }
  bool any_live = false;
  for (uint32_t j = 0; j < nj; j++) {
    out_job[j] = jst[j] == LB_OK ? 1 : -jst[j];
    any_live |= jst[j] == LB_OK;
  }
  if (any_live && !root_ok) {
    st = search_invalid(e, b, mu, out_job);
    if (st != LB_OK) return st;
  }
  if (e->profiling) hipEventRecord(e->ev1[ST_TOTAL], e->stream);
  finish_profile(e);
  return LB_OK;
}

extern "C" int32_t lb_batch_verify(lb_engine* e, lb_batch* b, const uint64_t* scalars, int32_t* out_job) {
  if (!e || !b || (b->n_jobs && !out_job)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  return verify_locked(e, b, scalars, out_job);
}

extern "C" int32_t lb_batch_partial(lb_engine* e, lb_batch* b, const uint64_t* scalars, uint8_t* out576,
                                    int32_t* out_job) {
  if (!e || !b || !out576 || (b->n_jobs && !out_job)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  uint32_t m = 1, mu = 1;
  if (b->n_jobs == 0) {
    fp12_to_be576(out576, fp12_one());
    return LB_OK;
  }
  busy_scope busy(e->device, e, e->latency);
  std::vector<int32_t> jst(b->n_jobs);
  for (bool per_set = false;; per_set = true) {  // (as verify_locked)
    int32_t st = run_pipeline(e, b, scalars, m, mu, false, per_set);  // always blinded: multiplied with other partials
    if (st != LB_OK) return st;
    LB_HIP(e->parts.ensure(576));
    {
      stage_scope sc(e, ST_ROOT, e->stream);
      hipLaunchKernelGGL(e->plan.fe == FE_ROW ? k_root_partial_row : k_root_partial, dim3(1), dim3(e->plan.fe == FE_ROW ? LBR_NT : 64), 0, e->stream, mu, e->treeP.as<uint32_t>(),
                         e->fS.as<uint32_t>(), e->parts.as<uint8_t>());
    }
    LB_HIP(hipGetLastError());
    uint32_t sgb_flag[2] = {0u, 0u};
    LB_HIP(hipMemcpyAsync(out576, e->parts.p, 576, hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipMemcpyAsync(jst.data(), e->job_status.p, (size_t)b->n_jobs * 4, hipMemcpyDeviceToHost, e->stream));
    if (e->sgb_active) LB_HIP(hipMemcpyAsync(sgb_flag, e->sgb_flag.p, 8, hipMemcpyDeviceToHost, e->stream));
    if (e->profiling) hipEventRecord(e->ev1[ST_TOTAL], e->stream);
    LB_HIP(hipStreamSynchronize(e->stream));
    if (!sgb_failed(e, sgb_flag)) break;
  }
  for (uint32_t j = 0; j < b->n_jobs; j++) out_job[j] = jst[j] == LB_OK ? 1 : -jst[j];
  finish_profile(e);
  e->partial_serial = b->serial;
  e->partial_mu = mu;
  return LB_OK;
}

extern "C" int32_t lb_batch_search_after_partial(lb_engine* e, lb_batch* b, int32_t* out_job) {
  if (!e || !b || (b->n_jobs && !out_job)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  if (b->n_jobs == 0) return LB_OK;
  if (e->partial_serial == 0 || e->partial_serial != b->serial) return LB_ERR_ARGUMENT;  // another call ran since
  LB_HIP(hipSetDevice(e->device));
  busy_scope busy(e->device, e, e->latency);
  const uint32_t mu = e->partial_mu, nj = b->n_jobs;
  LB_HIP(e->verdict.ensure(4));
  LB_HIP(e->y_root.ensure(576));
  // this shard's own root check: a passing shard is done, a failing one searches from it
  hipLaunchKernelGGL(e->plan.fe == FE_ROW ? k_root_check_row : k_root_check, dim3(1), dim3(e->plan.fe == FE_ROW ? LBR_NT : 64), 0, e->stream, mu, e->treeP.as<uint32_t>(), e->fS.as<uint32_t>(),
                     e->verdict.as<int32_t>(), e->y_root.as<uint32_t>());
  LB_HIP(hipGetLastError());
  std::vector<int32_t> jst(nj);
  int32_t root_ok = 0;
  LB_HIP(hipMemcpyAsync(jst.data(), e->job_status.p, (size_t)nj * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(&root_ok, e->verdict.p, 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  bool any_live = false;
  for (uint32_t j = 0; j < nj; j++) {
    out_job[j] = jst[j] == LB_OK ? 1 : -jst[j];
    any_live |= jst[j] == LB_OK;
  }
  int32_t st = LB_OK;
  if (any_live && !root_ok) st = search_invalid(e, b, mu, out_job);
  e->partial_serial = 0;
  return st;
}

extern "C" int32_t lb_fp12_product_is_one(lb_engine* e, const uint8_t* partials576, uint32_t n, int32_t* ok) {
  if (!e || !ok || (n && !partials576)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  LB_HIP(e->parts.ensure((size_t)(n ? n : 1) * 576));
  LB_HIP(e->ok.ensure(4));
  if (n) LB_HIP(hipMemcpyAsync(e->parts.p, partials576, (size_t)n * 576, hipMemcpyHostToDevice, e->stream));
  const bool prow = pipe_fe_form(e->knobs, device_alone(e)) == FE_ROW;
  hipLaunchKernelGGL(prow ? k_partials_check_row : k_partials_check, dim3(1), dim3(prow ? LBR_NT : 64), 0, e->stream, n, e->parts.as<uint8_t>(),
                     e->ok.as<int32_t>());
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(ok, e->ok.p, 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// upload into the engine-owned workspace batch + verify, under one hold of the engine lock
static int32_t verify_jobs_ws(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                              const uint32_t* set_pk_offsets, const uint8_t* pubkeys, const uint32_t* pk_indices,
                              const uint8_t* signing_roots, const uint8_t* signatures, const uint32_t* sig_sizes,
                              const uint64_t* scalars, int32_t* out_job) {
  if (!e || !job_offsets || (n_jobs && !out_job)) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->scratch) e->scratch = new lb_batch();
  int32_t st = batch_fill(e, e->scratch, n_jobs, job_offsets, set_pk_offsets, pubkeys, pk_indices, signing_roots,
                          signatures, sig_sizes);
  if (st != LB_OK) return st;
  return verify_locked(e, e->scratch, scalars, out_job);
}

extern "C" int32_t lb_verify_jobs(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                                  const uint32_t* set_pk_offsets, const uint8_t* pubkeys,
                                  const uint8_t* signing_roots, const uint8_t* signatures,
                                  const uint32_t* sig_sizes, const uint64_t* scalars, int32_t* out_job) {
  return verify_jobs_ws(e, n_jobs, job_offsets, set_pk_offsets, pubkeys, nullptr, signing_roots, signatures,
                        sig_sizes, scalars, out_job);
}

extern "C" int32_t lb_verify_jobs_indexed(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                                          const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                                          const uint8_t* signing_roots, const uint8_t* signatures,
                                          const uint32_t* sig_sizes, const uint64_t* scalars, int32_t* out_job) {
  if (!pk_indices) {
    const int32_t st = check_null_indices(n_jobs, job_offsets, set_pk_offsets);
    if (st != LB_OK) return st;
    pk_indices = kNoIndices;
  }
  return verify_jobs_ws(e, n_jobs, job_offsets, set_pk_offsets, nullptr, pk_indices, signing_roots, signatures,
                        sig_sizes, scalars, out_job);
}

extern "C" int32_t lb_aggregate_pubkeys(lb_engine* e, uint32_t n_sets, const uint32_t* set_pk_offsets,
                                        const uint8_t* pubkeys, uint8_t* out96, int32_t* out_status) {
  if (!e || !set_pk_offsets || (n_sets && (!out96 || !out_status))) return LB_ERR_ARGUMENT;
  if (set_pk_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t i = 0; i < n_sets; i++)
    if (set_pk_offsets[i + 1] < set_pk_offsets[i]) return LB_ERR_ARGUMENT;
  uint32_t n_pks = set_pk_offsets[n_sets];
  if (n_pks && !pubkeys) return LB_ERR_ARGUMENT;
  if (!n_sets) return LB_OK;
  if (n_pks & LB_CHUNK_FIRST) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  // the batch pipeline's chunk decomposition (<= LB_PK_CHUNK keys, flagged set starts): chunk sums
  // combined by the wave tree in k_pk_chunks, then k_pk_out96 per set
  std::vector<uint32_t> sco(n_sets + 1), clo;
  for (uint32_t i = 0; i < n_sets; i++) {
    sco[i] = (uint32_t)clo.size();
    for (uint32_t k = set_pk_offsets[i]; k < set_pk_offsets[i + 1]; k += LB_PK_CHUNK)
      clo.push_back(k | (k == set_pk_offsets[i] ? LB_CHUNK_FIRST : 0u));
  }
  sco[n_sets] = (uint32_t)clo.size();
  const uint32_t nc = (uint32_t)clo.size();
  clo.push_back(n_pks | LB_CHUNK_FIRST);
  dbuf dsco, dclo, pk, acc, cst, out, stat;
  hipError_t r = dsco.ensure(sco.size() * 4);
  if (r == hipSuccess) r = dclo.ensure(clo.size() * 4);
  if (r == hipSuccess) r = pk.ensure((size_t)(n_pks ? n_pks : 1) * 96);
  if (r == hipSuccess) r = acc.ensure((size_t)(nc ? nc : 1) * sizeof(g1j));
  if (r == hipSuccess) r = cst.ensure((size_t)(nc ? nc : 1) * 4);
  if (r == hipSuccess) r = out.ensure((size_t)n_sets * 96);
  if (r == hipSuccess) r = stat.ensure((size_t)n_sets * 4);
  if (r == hipSuccess) r = hipMemcpyAsync(dsco.p, sco.data(), sco.size() * 4, hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess) r = hipMemcpyAsync(dclo.p, clo.data(), clo.size() * 4, hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess && n_pks) r = hipMemcpyAsync(pk.p, pubkeys, (size_t)n_pks * 96, hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess) {
    if (nc)
      hipLaunchKernelGGL(k_pk_chunks, dim3(nblk(nc)), dim3(LB_TPB), 0, e->stream, nc, dclo.as<uint32_t>(), pk.as<uint8_t>(),
                         acc.as<uint32_t>(), cst.as<int32_t>());
    hipLaunchKernelGGL(k_pk_out96, dim3(nblk(n_sets)), dim3(LB_TPB), 0, e->stream, n_sets, nc, dsco.as<uint32_t>(),
                       acc.as<uint32_t>(), cst.as<int32_t>(), out.as<uint8_t>(), stat.as<int32_t>());
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(out96, out.p, (size_t)n_sets * 96, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipMemcpyAsync(out_status, stat.p, (size_t)n_sets * 4, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  dbuf* tmp[] = {&dsco, &dclo, &pk, &acc, &cst, &out, &stat};
  for (dbuf* d : tmp) d->release();
  if (r != hipSuccess) {
    fprintf(stderr, "lodestar_bls: aggregate failed: %s\n", hipGetErrorString(r));
    return LB_ERR_DEVICE;
  }
  return LB_OK;
}

extern "C" int32_t lb_aggregate_signatures(lb_engine* e, uint32_t n_groups, const uint32_t* group_offsets,
                                           const uint8_t* sigs96, const uint32_t* sig_sizes, int32_t validate,
                                           uint8_t* out96, int32_t* out_status) {
  if (!e || !group_offsets || (n_groups && (!out96 || !out_status))) return LB_ERR_ARGUMENT;
  if (group_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t g = 0; g < n_groups; g++)
    if (group_offsets[g + 1] < group_offsets[g]) return LB_ERR_ARGUMENT;
  const uint32_t n = group_offsets[n_groups];
  if (n && !sigs96) return LB_ERR_ARGUMENT;
  if (!n_groups) return LB_OK;
  // chunks of <= LB_PK_CHUNK signatures, never spanning groups
  std::vector<uint32_t> chunk_lo, group_chunk_off(n_groups + 1);
  for (uint32_t g = 0; g < n_groups; g++) {
    group_chunk_off[g] = (uint32_t)chunk_lo.size();
    for (uint32_t i = group_offsets[g]; i < group_offsets[g + 1]; i += LB_PK_CHUNK) chunk_lo.push_back(i);
  }
  group_chunk_off[n_groups] = (uint32_t)chunk_lo.size();
  const uint32_t nc = (uint32_t)chunk_lo.size();
  chunk_lo.push_back(n);
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  const uint32_t ns = n ? n : 1, ncs = nc ? nc : 1;
  dbuf in, sizes, aff, aos, inf, st, clo, goff, acc, cst, out, ost;
  hipError_t r = in.ensure((size_t)ns * 96);
  if (r == hipSuccess) r = sizes.ensure((size_t)ns * 4);
  if (r == hipSuccess) r = aff.ensure((size_t)ns * sizeof(g2a));
  if (r == hipSuccess) r = aos.ensure((size_t)ns * sizeof(g2a));
  if (r == hipSuccess) r = inf.ensure((size_t)ns * 4);
  if (r == hipSuccess) r = st.ensure((size_t)ns * 4);
  if (r == hipSuccess) r = clo.ensure((size_t)(nc + 1) * 4);
  if (r == hipSuccess) r = goff.ensure((size_t)(n_groups + 1) * 4);
  if (r == hipSuccess) r = acc.ensure((size_t)ncs * sizeof(g2j));
  if (r == hipSuccess) r = cst.ensure((size_t)ncs * 4);
  if (r == hipSuccess) r = out.ensure((size_t)n_groups * 96);
  if (r == hipSuccess) r = ost.ensure((size_t)n_groups * 4);
  hipStream_t s1 = e->stream;
  if (r == hipSuccess && n) r = hipMemcpyAsync(in.p, sigs96, (size_t)n * 96, hipMemcpyHostToDevice, s1);
  if (r == hipSuccess && n && sig_sizes) r = hipMemcpyAsync(sizes.p, sig_sizes, (size_t)n * 4, hipMemcpyHostToDevice, s1);
  if (r == hipSuccess) r = hipMemcpyAsync(clo.p, chunk_lo.data(), (size_t)(nc + 1) * 4, hipMemcpyHostToDevice, s1);
  if (r == hipSuccess)
    r = hipMemcpyAsync(goff.p, group_chunk_off.data(), (size_t)(n_groups + 1) * 4, hipMemcpyHostToDevice, s1);
  if (r == hipSuccess) {
    if (n) {
      hipLaunchKernelGGL(k_decompress_sigs, dim3(nblk(n)), dim3(LB_TPB), 0, s1, n, in.as<uint8_t>(),
                         sig_sizes ? sizes.as<uint32_t>() : nullptr, aff.as<uint32_t>(), aos.as<uint4>(),
                         inf.as<uint32_t>(), st.as<int32_t>());
      if (validate)
        hipLaunchKernelGGL(k_sig_subgroup, dim3(nblk(n)), dim3(LB_TPB), 0, s1, n, aff.as<uint32_t>(),
                           inf.as<uint32_t>(), st.as<int32_t>());
    }
    if (nc)
      hipLaunchKernelGGL(k_sig_agg_chunks, dim3(nblk(nc)), dim3(LB_TPB), 0, s1, nc, clo.as<uint32_t>(),
                         aff.as<uint32_t>(), n, inf.as<uint32_t>(), st.as<int32_t>(), acc.as<uint32_t>(),
                         cst.as<int32_t>());
    hipLaunchKernelGGL(k_sig_agg_groups, dim3(nblk(n_groups)), dim3(LB_TPB), 0, s1, n_groups, goff.as<uint32_t>(),
                       acc.as<uint32_t>(), nc, cst.as<int32_t>(), out.as<uint8_t>(), ost.as<int32_t>());
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(out96, out.p, (size_t)n_groups * 96, hipMemcpyDeviceToHost, s1);
  if (r == hipSuccess) r = hipMemcpyAsync(out_status, ost.p, (size_t)n_groups * 4, hipMemcpyDeviceToHost, s1);
  if (r == hipSuccess) r = hipStreamSynchronize(s1);
  dbuf* all[] = {&in, &sizes, &aff, &aos, &inf, &st, &clo, &goff, &acc, &cst, &out, &ost};
  for (dbuf* d : all) d->release();
  if (r != hipSuccess) {
    fprintf(stderr, "lodestar_bls: signature aggregation failed: %s\n", hipGetErrorString(r));
    return LB_ERR_DEVICE;
  }
  return LB_OK;
}

extern "C" int32_t lb_merkleize(lb_engine* e, uint32_t n_trees, const uint32_t* chunk_offsets, const uint8_t* chunks32,
                                const uint32_t* depths, const uint64_t* mix_lengths, uint8_t* out_roots32) {
  if (!e || !chunk_offsets || (n_trees && (!depths || !mix_lengths || !out_roots32))) return LB_ERR_ARGUMENT;
  if (chunk_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t t = 0; t < n_trees; t++) {
    const uint32_t len = chunk_offsets[t + 1] - chunk_offsets[t];
    if (chunk_offsets[t + 1] < chunk_offsets[t] || depths[t] > 63 || (depths[t] < 32 && len > (1u << depths[t])))
      return LB_ERR_ARGUMENT;
  }
  const uint32_t nc = chunk_offsets[n_trees];
  if (nc && !chunks32) return LB_ERR_ARGUMENT;
  if (!n_trees) return LB_OK;
  return run_simple(e, {{chunk_offsets, (size_t)(n_trees + 1) * 4, false, nullptr},
                        {depths, (size_t)n_trees * 4, false, nullptr},
                        {mix_lengths, (size_t)n_trees * 8, false, nullptr},
                        {chunks32, (size_t)nc * 32, false, nullptr},
                        {nullptr, 64 * 32, true, nullptr},  // zero-subtree roots (device scratch)
                        {nullptr, (size_t)n_trees * 32, true, out_roots32}},
                    [&](std::vector<void*>& p) {
                      hipLaunchKernelGGL(k_ssz_zero_hashes, dim3(1), dim3(64), 0, e->stream, (uint8_t*)p[4]);
                      hipLaunchKernelGGL(k_merkleize, dim3(nblk(n_trees)), dim3(LB_TPB), 0, e->stream, n_trees,
                                         (const uint32_t*)p[0], (const uint32_t*)p[1], (const uint64_t*)p[2],
                                         (uint8_t*)p[3], (const uint8_t*)p[4], (uint8_t*)p[5]);
                    });
}

// A segment's signature sets from the blocks' SSZ bytes (lb_ssz_walk.h, lb_ssz_sets.h): one upload
// (the per-block arguments, the domains and the bytes in one buffer), a launch sequence that
// depends on nothing read back, one download, one synchronisation.
extern "C" int32_t lb_block_sets_from_ssz(lb_engine* e, uint32_t n_blocks, const uint32_t* byte_offsets,
                                          const uint8_t* ssz, const uint32_t* forks, const uint8_t* domains32,
                                          const uint64_t* fork_epochs, const uint64_t* state_slots, uint32_t flags,
                                          int32_t* out_status, uint32_t* out_n_sets, uint32_t* out_kind,
                                          uint8_t* out_roots32, uint8_t* out_sigs96, uint64_t* out_ref) {
  if (!e) return LB_ERR_ARGUMENT;
  if (!n_blocks) return LB_OK;
  if (n_blocks > 64 || !byte_offsets || !forks || !domains32 || !fork_epochs || !state_slots || !out_status ||
      !out_n_sets || !out_kind || !out_roots32 || !out_sigs96 || !out_ref)
    return LB_ERR_ARGUMENT;
  if (byte_offsets[0] != 0) return LB_ERR_ARGUMENT;
  for (uint32_t b = 0; b < n_blocks; b++)
    if (byte_offsets[b + 1] < byte_offsets[b] || forks[b] > SSZ_CAPELLA) return LB_ERR_ARGUMENT;
  const uint32_t total = byte_offsets[n_blocks];
  if (total > (64u << 20) || (total && !ssz)) return LB_ERR_ARGUMENT;
  const bool skip = (flags & 1u) != 0;
  const size_t rows = (size_t)n_blocks * LB_SSZ_MAX_SETS;
  // upload: arguments | domains | bytes
  const size_t up_dom = (size_t)n_blocks * sizeof(ssz_blk_arg), up_ssz = up_dom + (size_t)n_blocks * 384;
  const size_t up_bytes = up_ssz + total;
  // work area: zero-subtree roots | indices | nodes | fold buffers (A and B per block)
  const size_t w_blk = 64 * 32, w_nodes = w_blk + (((size_t)n_blocks * sizeof(ssz_blk) + 31) & ~(size_t)31);
  const size_t w_fold = w_nodes + (size_t)n_blocks * LB_SSZ_N_NODES * 32;
  // download: ref | roots | signatures | kind | status | set counts
  const size_t d_roots = rows * 32, d_sigs = d_roots + rows * 32, d_kind = d_sigs + rows * 96;
  const size_t d_status = d_kind + rows * 4, d_nsets = d_status + (size_t)n_blocks * 4;
  const size_t down_bytes = d_nsets + (size_t)n_blocks * 4;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  e->ssz_up.resize(up_bytes);
  ssz_blk_arg* args = reinterpret_cast<ssz_blk_arg*>(e->ssz_up.data());
  uint64_t fold_nodes = 0;
  for (uint32_t b = 0; b < n_blocks; b++) {
    args[b] = ssz_blk_arg{byte_offsets[b], byte_offsets[b + 1], forks[b], 0, fork_epochs[b], state_slots[b], fold_nodes};
    fold_nodes += 2 * (uint64_t)ssz_fold_cap(byte_offsets[b + 1] - byte_offsets[b]);
  }
  memcpy(e->ssz_up.data() + up_dom, domains32, (size_t)n_blocks * 384);
  if (total) memcpy(e->ssz_up.data() + up_ssz, ssz, total);
  e->ssz_down.resize(down_bytes);
  const size_t work_cap = e->ssz_work.cap;
  LB_HIP(e->ssz_in.ensure(up_bytes + 64));  // the walk never reads past a block's end; slack all the same
  LB_HIP(e->ssz_work.ensure(w_fold + fold_nodes * 32));
  LB_HIP(e->ssz_out.ensure(down_bytes));
  if (e->ssz_work.cap != work_cap) e->ssz_zh_ready = false;  // a new allocation (maybe at the old address)
  hipStream_t s1 = e->stream;
  uint8_t* in = e->ssz_in.as<uint8_t>();
  uint8_t* work = e->ssz_work.as<uint8_t>();
  uint8_t* out = e->ssz_out.as<uint8_t>();
  const ssz_blk_arg* d_args = reinterpret_cast<const ssz_blk_arg*>(in);
  ssz_blk* d_blks = reinterpret_cast<ssz_blk*>(work + w_blk);
  uint32_t* d_nodes = reinterpret_cast<uint32_t*>(work + w_nodes);
  LB_HIP(hipMemcpyAsync(in, e->ssz_up.data(), up_bytes, hipMemcpyHostToDevice, s1));
  LB_HIP(hipMemsetAsync(out, 0, down_bytes, s1));
  if (!e->ssz_zh_ready) hipLaunchKernelGGL(k_ssz_zero_hashes, dim3(1), dim3(64), 0, s1, work);
  hipLaunchKernelGGL(k_ssz_index, dim3(n_blocks), dim3(LB_SSZ_WG), 0, s1, n_blocks, d_args, in + up_ssz, skip ? 1u : 0u,
                     d_blks, reinterpret_cast<int32_t*>(out + d_status), reinterpret_cast<uint32_t*>(out + d_nsets));
  if (!skip)
    hipLaunchKernelGGL(k_ssz_block_root, dim3(n_blocks), dim3(LB_SSZ_WG), 0, s1, n_blocks, d_args, in + up_ssz, d_blks,
                       d_nodes, reinterpret_cast<uint32_t*>(work + w_fold), work);
  hipLaunchKernelGGL(k_ssz_sets, dim3(nblk((uint32_t)rows)), dim3(LB_TPB), 0, s1, n_blocks, d_args, in + up_ssz,
                     in + up_dom, skip ? 1u : 0u, d_blks, reinterpret_cast<const uint32_t*>(out + d_nsets), d_nodes, work,
                     reinterpret_cast<uint32_t*>(out + d_kind), out + d_roots, out + d_sigs,
                     reinterpret_cast<uint64_t*>(out));
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(e->ssz_down.data(), out, down_bytes, hipMemcpyDeviceToHost, s1));
  e->ssz_syncs++;
  LB_HIP(hipStreamSynchronize(s1));
  e->ssz_zh_ready = true;
  const uint8_t* dn = e->ssz_down.data();
  memcpy(out_ref, dn, rows * 32);
  memcpy(out_roots32, dn + d_roots, rows * 32);
  memcpy(out_sigs96, dn + d_sigs, rows * 96);
  memcpy(out_kind, dn + d_kind, rows * 4);
  memcpy(out_status, dn + d_status, (size_t)n_blocks * 4);
  memcpy(out_n_sets, dn + d_nsets, (size_t)n_blocks * 4);
  return LB_OK;
}

extern "C" uint64_t lb_block_sets_syncs(const lb_engine* e) { return e ? e->ssz_syncs : 0; }

extern "C" int32_t lb_g1_decompress(lb_engine* e, uint32_t n, const uint8_t* in48, uint8_t* out96,
                                    int32_t* out_status, int32_t validate) {
  if (!e || (n && (!in48 || !out96 || !out_status))) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  return run_simple(e, {{in48, (size_t)n * 48, false, nullptr}, {nullptr, (size_t)n * 96, true, out96},
                        {nullptr, (size_t)n * 4, true, out_status}},
                    [&](std::vector<void*>& p) {
                      hipLaunchKernelGGL(k_g1_decompress, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n,
                                         (const uint8_t*)p[0], (uint8_t*)p[1], (int32_t*)p[2], validate);
                    });
}

extern "C" int32_t lb_sk_to_pk(lb_engine* e, uint32_t n, const uint8_t* sks32, uint8_t* out48, uint8_t* out96) {
  if (!e || (n && !sks32)) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  return run_simple(e, {{sks32, (size_t)n * 32, false, nullptr}, {nullptr, (size_t)n * 48, true, out48},
                        {nullptr, (size_t)n * 96, true, out96}},
                    [&](std::vector<void*>& p) {
                      hipLaunchKernelGGL(k_sk_to_pk, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n,
                                         (const uint8_t*)p[0], (uint8_t*)p[1], (uint8_t*)p[2]);
                    });
}

extern "C" int32_t lb_sign(lb_engine* e, uint32_t n, const uint8_t* sks32, const uint8_t* msgs32, uint8_t* out96) {
  if (!e || (n && (!sks32 || !msgs32 || !out96))) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  return run_simple(e, {{sks32, (size_t)n * 32, false, nullptr}, {msgs32, (size_t)n * 32, false, nullptr},
                        {nullptr, (size_t)n * 96, true, out96}},
                    [&](std::vector<void*>& p) {
                      hipLaunchKernelGGL(k_sign, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n,
                                         (const uint8_t*)p[0], (const uint8_t*)p[1], (uint8_t*)p[2]);
                    });
}
