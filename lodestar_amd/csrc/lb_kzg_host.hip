// The KZG calls of the C ABI (include/lodestar_bls.h lb_kzg_*, lb_g1_lincomb): host orchestration
// of the kernels of lb_kzg.h, lb_kzg_field.h and lb_kzg_fk20.h on the engine's stream s1.  Like
// lb_engine.hip it is compiled with -DLB_KGROUP=99 (no kernel definitions) and launches through
// lb_kdecl.h.  Every call holds the engine's mutex, takes its device buffers from a kzg_bufs that
// frees them on every way out, and states its stages in order; the stages that several calls share
// (decode, transforms, the setup's linear combinations, the status fold) are the helpers below.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include "lb_kzg.h"
#include "lb_kzg_field.h"
#include "lb_kzg_fk20.h"
#include "lb_kzg_transcript.h"
#include "lb_kzg_host.h"
#include "lb_engine_impl.h"
#include "lb_kdecl.h"  // kernels of the other translation units (split build)

extern "C" int32_t lb_kzg_load_setup(lb_engine* e, const uint8_t* g1_48, uint32_t n_g1, const uint8_t* g2_96,
                                     uint32_t n_g2, int32_t* out_status) {
  if (!e || !n_g1 || !g1_48 || !g2_96 || n_g2 < 2 || !out_status) return LB_ERR_ARGUMENT;
  // [tau^0] G2, [tau^1] G2 and, where the setup reaches it, [tau^64] G2 (the cell calls), side by side
  const uint32_t n2 = n_g2 >= 65 ? 3 : 2;
  std::vector<uint8_t> g2in((size_t)n2 * 96);
  memcpy(g2in.data(), g2_96, 2 * 96);
  if (n2 == 3) memcpy(g2in.data() + 2 * 96, g2_96 + (size_t)64 * 96, 96);
  std::vector<int32_t> st2(3, LB_OK);
  kzg_state& kz = e->kzg;
  kz.cells = false;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    LB_HIP(hipSetDevice(e->device));
    kz.fk_ready = false;  // the FK20 table belongs to the setup it was built from
    kz.fk_x.release();
    LB_HIP(kz.g1.ensure((size_t)n_g1 * sizeof(g1a)));
    LB_HIP(kz.g2.ensure(3 * sizeof(g2a)));
  }
  const int32_t r =
      run_simple(e, {{g1_48, (size_t)n_g1 * 48, false, nullptr}, {nullptr, (size_t)n_g1 * 4, true, out_status},
                     {g2in.data(), g2in.size(), false, nullptr}, {nullptr, (size_t)n2 * 4, true, st2.data()}},
                 [&](std::vector<void*>& p) {
                   hipLaunchKernelGGL(k_kzg_setup_g1, dim3(nblk(n_g1)), dim3(LB_TPB), 0, e->stream, n_g1,
                                      (const uint8_t*)p[0], kz.g1.as<uint32_t>(), n_g1, (int32_t*)p[1]);
                   hipLaunchKernelGGL(k_kzg_setup_g2, dim3(1), dim3(64), 0, e->stream, n2, (const uint8_t*)p[2],
                                      kz.g2.as<uint32_t>(), (int32_t*)p[3]);
                 });
  if (r != LB_OK) return r;
  if (st2[0] != LB_OK || st2[1] != LB_OK || st2[2] != LB_OK) {
    kz.n = 0;
    return st2[0] != LB_OK ? st2[0] : (st2[1] != LB_OK ? st2[1] : st2[2]);
  }
  for (uint32_t i = 0; i < n_g1; i++)
    if (out_status[i] != LB_OK) {
      kz.n = 0;
      return out_status[i];
    }
  {
    // the blob-level calls' inverse-transform table (lb_fr.h), computed here on the host
    std::vector<fr> tw(LB_FR_TW_LEN);
    fr_intt_table(tw.data(), LB_FR_LOGN);
    std::lock_guard<std::mutex> lk(e->mu);
    LB_HIP(hipSetDevice(e->device));
    LB_HIP(kz.tw.ensure(tw.size() * sizeof(fr)));
    LB_HIP(hipMemcpyAsync(kz.tw.p, tw.data(), tw.size() * sizeof(fr), hipMemcpyHostToDevice, e->stream));
    // the cell calls' tables beside it: forward twiddles, w^j, w^-m, the 64-point inverse table
    std::vector<fr> ct(LB_FR_CELL_TAB_LEN);
    fr_cell_tables(ct.data());
    kz.h64.resize(LB_FR_CELLS);
    for (uint32_t i = 0; i < LB_FR_CELLS; i++) kz.h64[i] = ct[LB_FR_CELL_TAB_WINV + fr_cell_h64_index(i)];
    LB_HIP(kz.cell_tab.ensure(ct.size() * sizeof(fr)));
    LB_HIP(hipMemcpyAsync(kz.cell_tab.p, ct.data(), ct.size() * sizeof(fr), hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    kz.fk_ready = false;  // ... also one that a call built while this load was under way
  }
  kz.n = n_g1;
  kz.cells = n2 == 3;
  return LB_OK;
}

// The launches of out48 = compress(sum_i s_i P_i) over device buffers: P_i = setup point i
// (d_pts48 null) or n compressed points; d_scalars n x 8 LE words; d_terms n and d_part
// ceil(n / 64) g1j (SoA); d_status n codes (LB_OK for setup points).  n >= 1.
static void g1_lincomb_launch(lb_engine* e, uint32_t n, const uint8_t* d_pts48, const uint32_t* d_scalars,
                              uint32_t* d_terms, uint32_t* d_part, int32_t* d_status, uint8_t* d_out48) {
  hipLaunchKernelGGL(k_g1_terms, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n, d_pts48, e->kzg.g1.as<uint32_t>(),
                     e->kzg.n, d_scalars, d_terms, d_status);
  // reduce 64:1 per level, ping-ponging between the term buffer and the partials buffer
  uint32_t* bufs[2] = {d_terms, d_part};
  uint32_t m = n;
  int cur = 0;
  while (m > 1) {
    const uint32_t mo = (m + 63) / 64;
    hipLaunchKernelGGL(k_g1_sum64, dim3(mo), dim3(64), 0, e->stream, m, bufs[cur], mo, bufs[cur ^ 1]);
    m = mo;
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_g1_out48, dim3(1), dim3(64), 0, e->stream, bufs[cur], m, d_out48);
}

extern "C" int32_t lb_g1_lincomb(lb_engine* e, uint32_t n, const uint8_t* points48, const uint8_t* scalars32,
                                 uint8_t* out48) {
  if (!e || !out48 || (n && !scalars32)) return LB_ERR_ARGUMENT;
  if (!points48 && n > e->kzg.n) return LB_ERR_ARGUMENT;
  if (!n) {  // empty sum: infinity
    memset(out48, 0, 48);
    out48[0] = 0xc0;
    return LB_OK;
  }
  const uint32_t n1 = (n + 63) / 64;
  std::vector<int32_t> st(n, LB_OK);
  const int32_t r = run_simple(
      e, {{points48, points48 ? (size_t)n * 48 : 0, false, nullptr}, {scalars32, (size_t)n * 32, false, nullptr},
          {nullptr, (size_t)n * sizeof(g1j), true, nullptr}, {nullptr, (size_t)n1 * sizeof(g1j), true, nullptr},
          {nullptr, (size_t)n * 4, true, st.data()}, {nullptr, 48, true, out48}},
      [&](std::vector<void*>& p) {
        g1_lincomb_launch(e, n, points48 ? (const uint8_t*)p[0] : nullptr, (const uint32_t*)p[1], (uint32_t*)p[2],
                          (uint32_t*)p[3], (int32_t*)p[4], (uint8_t*)p[5]);
      });
  if (r != LB_OK) return r;
  for (uint32_t i = 0; i < n; i++)
    if (st[i] != LB_OK) return st[i];
  return LB_OK;
}

extern "C" int32_t lb_kzg_verify_proof(lb_engine* e, const uint8_t* commitment48, const uint8_t* z32,
                                       const uint8_t* y32, const uint8_t* proof48, int32_t* ok) {
  if (!e || !commitment48 || !z32 || !y32 || !proof48 || !ok) return LB_ERR_ARGUMENT;
  if (e->kzg.n == 0) return LB_ERR_ARGUMENT;  // no setup loaded
  uint8_t io[96];
  memcpy(io, commitment48, 48);
  memcpy(io + 48, proof48, 48);
  uint8_t yz[64];
  memcpy(yz, y32, 32);
  memcpy(yz + 32, z32, 32);
  return run_simple(e, {{io, 96, false, nullptr}, {yz, 64, false, nullptr}, {nullptr, 4, true, ok}},
                    [&](std::vector<void*>& p) {
                      hipLaunchKernelGGL(k_kzg_check, dim3(1), dim3(64), 0, e->stream, (const uint8_t*)p[0],
                                         (const uint32_t*)p[1], e->kzg.g2.as<uint32_t>(), (int32_t*)p[2]);
                    });
}

// ---------------------------------------------------------------- the stages the blob-level calls share
namespace {
constexpr size_t kBlobBytes = (size_t)LB_FR_N * 32;
// the compressed G1 generator: the point whose scalar is y in the batched checks' k_g1_terms launch
const uint8_t kG1Gen48[48] = {0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c,
                              0x4f, 0xa9, 0xac, 0x0f, 0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05,
                              0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58, 0x6c, 0x55, 0xe8, 0x3f,
                              0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};

#define LB_TRY(call)                  \
  do {                                \
    const int32_t _rc = (call);       \
    if (_rc != LB_OK) return _rc;     \
  } while (0)

bool kzg_ready(const lb_engine* e) { return e && e->kzg.n == LB_FR_N && e->kzg.tw.p; }

// host threads that hash the per-blob challenges: LB_KZG_HASH_THREADS, default 8, 1 .. 16
uint32_t kzg_hash_threads() {
  const char* s = getenv("LB_KZG_HASH_THREADS");
  const long v = s && *s ? strtol(s, nullptr, 10) : 8;
  return (uint32_t)std::min<long>(16, std::max<long>(1, v));
}

// host hashing time (lb_kzg_batch_hash_ns): t0 = kzg_clock::now() before, kzg_ns_since(t0) after
using kzg_clock = std::chrono::steady_clock;
uint64_t kzg_ns_since(const kzg_clock::time_point& t0) {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(kzg_clock::now() - t0).count();
}

// The device buffers of one call, freed when it returns, whichever way.  get() after a failed
// allocation returns null without allocating; a call checks error() once per group of buffers, before
// it uses them.  Field elements are 8 words each.
struct kzg_bufs {
  std::vector<dbuf> owned;
  hipError_t err = hipSuccess;
  kzg_bufs() { owned.reserve(16); }
  kzg_bufs(const kzg_bufs&) = delete;
  kzg_bufs& operator=(const kzg_bufs&) = delete;
  ~kzg_bufs() {
    for (dbuf& b : owned) b.release();
  }
  template <class T>
  T* get(size_t bytes) {
    dbuf b;
    if (err == hipSuccess) err = b.ensure(bytes);
    if (b.p) owned.push_back(b);
    return b.as<T>();
  }
  hipError_t error() const { return err; }
};

// n blobs on the device: as given, as Montgomery Fr (k_fr_blob_load), and a status per blob
struct kzg_blobs {
  uint8_t* bytes;
  uint32_t* polys;
  int32_t* status;
  kzg_blobs(kzg_bufs& w, size_t n)
      : bytes(w.get<uint8_t>(n * kBlobBytes)), polys(w.get<uint32_t>(n * kBlobBytes)), status(w.get<int32_t>(n * 4)) {}
};
// upload n >= 1 blobs and decode them: d.status[b] = LB_OK / LB_BAD_SCALAR.  Does not synchronise.
int32_t kzg_decode_async(lb_engine* e, const kzg_blobs& d, uint32_t n, const uint8_t* blobs) {
  LB_HIP(hipMemcpyAsync(d.bytes, blobs, n * kBlobBytes, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemsetAsync(d.status, 0, (size_t)n * 4, e->stream));
  const uint32_t n_elems = n * LB_FR_N;
  hipLaunchKernelGGL(k_fr_blob_load, dim3((n_elems + 255) / 256), dim3(256), 0, e->stream, n_elems, d.bytes, d.polys,
                     d.status);
  LB_HIP(hipGetLastError());
  return LB_OK;
}
// ... and wait for the statuses: the calls that decide on them before going on
int32_t kzg_load_blobs(lb_engine* e, const kzg_blobs& d, uint32_t n, const uint8_t* blobs, std::vector<int32_t>& h_status) {
  LB_TRY(kzg_decode_async(e, d, n, blobs));
  h_status.assign(n, LB_OK);
  LB_HIP(hipMemcpyAsync(h_status.data(), d.status, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}
int32_t kzg_first_bad(const std::vector<int32_t>& st) {
  for (int32_t s : st)
    if (s != LB_OK) return s;
  return LB_OK;
}

// n_polys polynomials of evaluations -> coefficients (one workgroup each, the polynomial in LDS)
int32_t kzg_intt(lb_engine* e, uint32_t n_polys, const uint32_t* in, uint32_t* out_mont, uint32_t* out_le) {
  LB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fr_intt4096), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)LB_FR_INTT_LDS));
  hipLaunchKernelGGL(k_fr_intt4096, dim3(n_polys), dim3(LB_FR_WG), LB_FR_INTT_LDS, e->stream, in,
                     e->kzg.tw.as<uint32_t>(), out_mont, out_le);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

// n blobs' coefficients -> their 128 cells each (one workgroup per blob; d_blob_bytes: the blobs as
// given, which are the cells' first half)
int32_t kzg_coset_ntt(lb_engine* e, uint32_t n, const uint32_t* d_coef, const uint8_t* d_blob_bytes, uint8_t* d_cells) {
  LB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fr_coset_ntt4096),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)LB_FR_INTT_LDS));
  hipLaunchKernelGGL(k_fr_coset_ntt4096, dim3(n), dim3(LB_FR_WG), LB_FR_INTT_LDS, e->stream, d_coef, d_blob_bytes,
                     e->kzg.cell_tab.as<uint32_t>(), d_cells);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

// scratch of one 4096-term g1_lincomb_launch, shared by all of a call's
struct kzg_lincomb_ws {
  uint32_t* terms;
  uint32_t* part;
  int32_t* status;
  explicit kzg_lincomb_ws(kzg_bufs& w)
      : terms(w.get<uint32_t>((size_t)LB_FR_N * sizeof(g1j))), part(w.get<uint32_t>((size_t)(LB_FR_N / 64) * sizeof(g1j))),
        status(w.get<int32_t>((size_t)LB_FR_N * 4)) {}
};
// n vectors of 4096 LE scalars -> n compressed points: one linear combination of the setup each
int32_t kzg_setup_lincombs(lb_engine* e, const kzg_lincomb_ws& s, uint32_t n, const uint32_t* d_scalars,
                           uint8_t* d_out48) {
  for (uint32_t b = 0; b < n; b++)
    g1_lincomb_launch(e, LB_FR_N, nullptr, d_scalars + (size_t)b * LB_FR_N * 8, s.terms, s.part, s.status,
                      d_out48 + (size_t)48 * b);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

// commitments of n decoded blobs -> d_out48: their coefficients as LE scalars (d_coef_le, n blobs'
// worth), then one linear combination each
int32_t kzg_commit(lb_engine* e, const kzg_lincomb_ws& s, uint32_t n, const uint32_t* d_polys, uint32_t* d_coef_le,
                   uint8_t* d_out48) {
  LB_TRY(kzg_intt(e, n, d_polys, nullptr, d_coef_le));
  return kzg_setup_lincombs(e, s, n, d_coef_le, d_out48);
}

// evaluations `evals` (Montgomery, device) and the point z -> y = p(z) as LE words at d_y and the
// quotient's scalars at d_quot_le (one blob's worth); if d_proof48, also the proof = commitment to
// the quotient
int32_t kzg_open(lb_engine* e, kzg_bufs& w, const kzg_lincomb_ws& s, const uint32_t* evals, const fr& z,
                 uint32_t* d_quot_le, uint32_t* d_y, uint8_t* d_proof48) {
  uint32_t* d_coef = w.get<uint32_t>(kBlobBytes);
  uint32_t* d_z = w.get<uint32_t>(sizeof(fr));
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(d_z, &z, sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_TRY(kzg_intt(e, 1, evals, d_coef, nullptr));
  hipLaunchKernelGGL(k_fr_eval_quotient, dim3(1), dim3(LB_FR_WG), LB_FR_EQ_LDS, e->stream, d_coef, d_z, d_quot_le, d_y);
  LB_HIP(hipGetLastError());
  return d_proof48 ? kzg_setup_lincombs(e, s, 1, d_quot_le, d_proof48) : LB_OK;
}

// hash_to_bls_field(h || tag) of the aggregate form's transcript (lb_kzg_transcript.h has the per-blob forms')
fr kzg_hash_to_field(const uint8_t h[32], uint8_t tag) {
  sha_stream s;
  s.update(h, 32);
  s.update(&tag, 1);
  return kzg_digest_to_field(s);
}

// compute_challenges (lodestar_amd/kzg.py): transcript = domain || 4096 and n as 8-byte BE || the
// blobs' field elements (32-byte BE: a valid blob's own bytes) || the commitments;
// r = H(h || 0), x = H(h || 1)
void kzg_challenges(uint32_t n, const uint8_t* blobs, const uint8_t* commitments48, fr& r, fr& x) {
  sha_stream s;
  s.update(reinterpret_cast<const uint8_t*>("FSBLOBVERIFY_V1_"), 16);
  uint8_t be[16] = {0};
  be[6] = (uint8_t)(LB_FR_N >> 8);
  be[7] = (uint8_t)LB_FR_N;
  for (int i = 0; i < 4; i++) be[12 + i] = (uint8_t)(n >> (24 - 8 * i));
  s.update(be, 16);
  if (n) s.update(blobs, (size_t)n * LB_FR_N * 32);
  if (n) s.update(commitments48, (size_t)n * 48);
  uint8_t h[32];
  s.finish(h);
  r = kzg_hash_to_field(h, 0);
  x = kzg_hash_to_field(h, 1);
}

// sum_j r^j poly_j of n decoded blobs -> d_agg (allocated here); the powers also as LE scalars at
// d_pw_le (behind their Montgomery forms, one allocation)
int32_t kzg_aggregate(lb_engine* e, kzg_bufs& w, uint32_t n, const uint32_t* d_polys, const fr& r, uint32_t*& d_agg,
                      uint32_t*& d_pw_le) {
  std::vector<fr> pw(n), pw_le(n);
  fr p = fr_one();
  for (uint32_t j = 0; j < n; j++) {
    pw[j] = p;
    fr_to_le_words(pw_le[j].l, p);
    p = fr_mul(p, r);
  }
  uint32_t* d_pw = w.get<uint32_t>(2 * n * sizeof(fr));
  d_pw_le = d_pw + (size_t)8 * n;
  d_agg = w.get<uint32_t>(kBlobBytes);
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(d_pw, pw.data(), n * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_pw_le, pw_le.data(), n * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_fr_aggregate, dim3(LB_FR_N / 256), dim3(256), 0, e->stream, n, d_polys, d_pw, d_agg);
  LB_HIP(hipGetLastError());
  // pageable uploads return once staged, but pw / pw_le die with this frame: be safe
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}
}  // namespace

// ---------------------------------------------------------------- KZG, blob level (lb_kzg_field.h)
extern "C" int32_t lb_kzg_blob_to_commitment(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out48,
                                             int32_t* out_status) {
  if (!kzg_ready(e) || n_blobs > kMaxBlobs || (n_blobs && (!blobs || !out48 || !out_status))) return LB_ERR_ARGUMENT;
  if (!n_blobs) return LB_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, n_blobs);
  const kzg_lincomb_ws lin(w);
  uint32_t* d_coef_le = w.get<uint32_t>(n_blobs * kBlobBytes);
  uint8_t* d_commitments = w.get<uint8_t>((size_t)n_blobs * 48);
  LB_HIP(w.error());
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, n_blobs, blobs, blob_status));
  LB_TRY(kzg_commit(e, lin, n_blobs, d.polys, d_coef_le, d_commitments));
  LB_HIP(hipMemcpyAsync(out48, d_commitments, (size_t)n_blobs * 48, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  kzg_fold_status(n_blobs, blob_status.data(), nullptr, out_status, out48, 48);
  return LB_OK;
}

extern "C" int32_t lb_kzg_blob_coefficients(lb_engine* e, const uint8_t* blob, uint8_t* out_coeffs32le) {
  if (!kzg_ready(e) || !blob || !out_coeffs32le) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, 1);
  uint32_t* d_coef_le = w.get<uint32_t>(kBlobBytes);
  LB_HIP(w.error());
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, 1, blob, blob_status));
  if (blob_status[0] != LB_OK) return blob_status[0];
  LB_TRY(kzg_intt(e, 1, d.polys, nullptr, d_coef_le));
  LB_HIP(hipMemcpyAsync(out_coeffs32le, d_coef_le, kBlobBytes, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

extern "C" int32_t lb_kzg_compute_proof(lb_engine* e, const uint8_t* blob, const uint8_t* z32le, uint8_t* out_proof48,
                                        uint8_t* out_y32le) {
  if (!kzg_ready(e) || !blob || !z32le || !out_proof48 || !out_y32le) return LB_ERR_ARGUMENT;
  const fr zp = kzg_fr_from_le32(z32le);
  if (!fr_lt_mod(zp)) return LB_BAD_SCALAR;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, 1);
  const kzg_lincomb_ws lin(w);
  uint32_t* d_quot_le = w.get<uint32_t>(kBlobBytes);
  uint32_t* d_y = w.get<uint32_t>(sizeof(fr));
  uint8_t* d_proof = w.get<uint8_t>(48);
  LB_HIP(w.error());
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, 1, blob, blob_status));
  if (blob_status[0] != LB_OK) return blob_status[0];
  const fr z = fr_to_mont(zp);  // outlives the upload: the stream is synchronised below
  LB_TRY(kzg_open(e, w, lin, d.polys, z, d_quot_le, d_y, d_proof));
  LB_HIP(hipMemcpyAsync(out_proof48, d_proof, 48, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(out_y32le, d_y, 32, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

extern "C" int32_t lb_kzg_compute_aggregate_proof(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out48) {
  if (!kzg_ready(e) || n_blobs > kMaxBlobs || !out48 || (n_blobs && !blobs)) return LB_ERR_ARGUMENT;
  if (!n_blobs) {  // the zero polynomial's proof: infinity
    memset(out48, 0, 48);
    out48[0] = 0xc0;
    return LB_OK;
  }
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, n_blobs);
  const kzg_lincomb_ws lin(w);
  uint32_t* d_scalars = w.get<uint32_t>(n_blobs * kBlobBytes);  // the blobs' coefficients, then the quotient's
  uint8_t* d_commitments = w.get<uint8_t>((size_t)n_blobs * 48);
  uint32_t* d_y = w.get<uint32_t>(sizeof(fr));
  uint8_t* d_proof = w.get<uint8_t>(48);
  LB_HIP(w.error());
  // 1. the blobs, all valid, and their commitments, which the challenges hash
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, n_blobs, blobs, blob_status));
  LB_TRY(kzg_first_bad(blob_status));
  LB_TRY(kzg_commit(e, lin, n_blobs, d.polys, d_scalars, d_commitments));
  std::vector<uint8_t> comms((size_t)n_blobs * 48);
  LB_HIP(hipMemcpyAsync(comms.data(), d_commitments, comms.size(), hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  fr r, x;
  kzg_challenges(n_blobs, blobs, comms.data(), r, x);
  // 2. the aggregate polynomial and its opening at x
  uint32_t *d_agg, *d_pw_le;
  LB_TRY(kzg_aggregate(e, w, n_blobs, d.polys, r, d_agg, d_pw_le));
  LB_TRY(kzg_open(e, w, lin, d_agg, x, d_scalars, d_y, d_proof));
  LB_HIP(hipMemcpyAsync(out48, d_proof, 48, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

extern "C" int32_t lb_kzg_verify_aggregate_proof(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs,
                                                 const uint8_t* commitments48, const uint8_t* proof48, int32_t* ok) {
  if (!kzg_ready(e) || n_blobs > kMaxBlobs || !proof48 || !ok || (n_blobs && (!blobs || !commitments48)))
    return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  // k_kzg_check's inputs and output: y || x as LE words, C || proof, the verdict
  uint32_t* d_yx = w.get<uint32_t>(64);
  uint8_t* d_c_proof = w.get<uint8_t>(96);
  int32_t* d_ok = w.get<int32_t>(4);
  LB_HIP(w.error());
  fr r, x;
  if (!n_blobs) {
    // aggregated commitment = infinity, y = 0: e(proof, [tau - x] G2) == 1 iff the proof is infinity
    kzg_challenges(0, nullptr, nullptr, r, x);
    uint8_t inf48[48] = {0xc0};
    LB_HIP(hipMemcpyAsync(d_c_proof, inf48, 48, hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipMemsetAsync(d_yx, 0, 32, e->stream));
  } else {
    const kzg_blobs d(w, n_blobs);
    const kzg_lincomb_ws lin(w);
    uint32_t* d_quot_le = w.get<uint32_t>(kBlobBytes);  // the scan's quotient: not needed here
    uint8_t* d_commitments = w.get<uint8_t>((size_t)n_blobs * 48);
    LB_HIP(w.error());
    std::vector<int32_t> blob_status;
    LB_TRY(kzg_load_blobs(e, d, n_blobs, blobs, blob_status));
    LB_TRY(kzg_first_bad(blob_status));
    kzg_challenges(n_blobs, blobs, commitments48, r, x);
    uint32_t *d_agg, *d_pw_le;
    LB_TRY(kzg_aggregate(e, w, n_blobs, d.polys, r, d_agg, d_pw_le));
    LB_TRY(kzg_open(e, w, lin, d_agg, x, d_quot_le, d_yx, nullptr));  // y = agg(x)
    // C = sum r^j C_j; the commitments are curve- and subgroup-checked by k_g1_terms
    LB_HIP(hipMemcpyAsync(d_commitments, commitments48, (size_t)n_blobs * 48, hipMemcpyHostToDevice, e->stream));
    g1_lincomb_launch(e, n_blobs, d_commitments, d_pw_le, lin.terms, lin.part, lin.status, d_c_proof);
    LB_HIP(hipGetLastError());
    std::vector<int32_t> tst(n_blobs, LB_OK);
    LB_HIP(hipMemcpyAsync(tst.data(), lin.status, (size_t)n_blobs * 4, hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    if (const int32_t bad = kzg_first_bad(tst)) {
      *ok = -bad;
      return LB_OK;
    }
  }
  uint32_t x_le[8];
  fr_to_le_words(x_le, x);
  LB_HIP(hipMemcpyAsync(d_c_proof + 48, proof48, 48, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_yx + 8, x_le, 32, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_kzg_check, dim3(1), dim3(64), 0, e->stream, d_c_proof, d_yx, e->kzg.g2.as<uint32_t>(), d_ok);
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(ok, d_ok, 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// Many sidecars in one pass: every stage once over all of them, one synchronisation at the end.
// Device arrays in k_g1_terms' order: the commitments, then the proofs, then one G1 generator per
// sidecar; their scalars r_k^j, x_k from the host and y_k written by k_fr_eval_many.
extern "C" int32_t lb_kzg_verify_aggregate_proof_batch(lb_engine* e, uint32_t n, const uint32_t* blob_offsets,
                                                       const uint8_t* blobs, const uint8_t* commitments48,
                                                       const uint8_t* proofs48, int32_t* out_ok) {
  if (!kzg_ready(e) || n > kMaxGroups) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  if (!proofs48 || !out_ok || !kzg_offsets_ok(n, blob_offsets, kMaxBlobs)) return LB_ERR_ARGUMENT;
  const uint32_t nb = blob_offsets[n];
  if (nb && (!blobs || !commitments48)) return LB_ERR_ARGUMENT;
  const uint32_t n_pts = nb + 2 * n;
  const size_t nb1 = std::max<size_t>(nb, 1);
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, nb1);
  uint32_t* d_off = w.get<uint32_t>((size_t)(n + 1) * 4);
  uint32_t* d_pw = w.get<uint32_t>(nb1 * sizeof(fr));
  uint32_t* d_x = w.get<uint32_t>((size_t)n * sizeof(fr));
  uint32_t* d_agg = w.get<uint32_t>((size_t)n * kBlobBytes);
  uint32_t* d_coef = w.get<uint32_t>((size_t)n * kBlobBytes);
  uint8_t* d_pts = w.get<uint8_t>((size_t)n_pts * 48);
  uint32_t* d_scalars = w.get<uint32_t>((size_t)n_pts * 32);
  uint32_t* d_terms = w.get<uint32_t>((size_t)n_pts * sizeof(g1j));
  int32_t* d_term_status = w.get<int32_t>((size_t)n_pts * 4);
  int32_t* d_ok = w.get<int32_t>((size_t)n * 4);
  LB_HIP(w.error());
  // 1. the blobs go up and are decoded while the host hashes
  LB_HIP(hipMemcpyAsync(d_off, blob_offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
  if (nb) LB_TRY(kzg_decode_async(e, d, nb, blobs));
  // 2. challenges per sidecar; the host arrays live until the synchronisation below
  std::vector<fr> pw(nb1), xs(n), sc(nb + n);
  uint64_t hash_ns = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t lo = blob_offsets[k], cnt = blob_offsets[k + 1] - lo;
    fr r, x;
    const auto t0 = kzg_clock::now();
    kzg_challenges(cnt, cnt ? blobs + lo * kBlobBytes : nullptr, cnt ? commitments48 + (size_t)48 * lo : nullptr, r, x);
    hash_ns += kzg_ns_since(t0);
    fr p = fr_one();
    for (uint32_t j = 0; j < cnt; j++) {
      pw[lo + j] = p;
      fr_to_le_words(sc[lo + j].l, p);
      p = fr_mul(p, r);
    }
    xs[k] = x;
    fr_to_le_words(sc[nb + k].l, x);
  }
  e->kzg.batch_hash_ns = hash_ns;
  std::vector<uint8_t> pts((size_t)n_pts * 48);
  if (nb) memcpy(pts.data(), commitments48, (size_t)nb * 48);
  memcpy(pts.data() + (size_t)nb * 48, proofs48, (size_t)n * 48);
  for (uint32_t k = 0; k < n; k++) memcpy(pts.data() + (size_t)(nb + n + k) * 48, kG1Gen48, 48);
  if (nb) LB_HIP(hipMemcpyAsync(d_pw, pw.data(), (size_t)nb * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_x, xs.data(), (size_t)n * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_scalars, sc.data(), (size_t)(nb + n) * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_pts, pts.data(), pts.size(), hipMemcpyHostToDevice, e->stream));
  // 3. - 5. aggregates, their coefficients, their values y_k into the generators' scalar slots
  hipLaunchKernelGGL(k_fr_aggregate_seg, dim3(n * (LB_FR_N / 256)), dim3(256), 0, e->stream, n, d_off, nb, d.polys, d_pw,
                     d_agg);
  LB_HIP(hipGetLastError());
  LB_TRY(kzg_intt(e, n, d_agg, d_coef, nullptr));
  hipLaunchKernelGGL(k_fr_eval_many, dim3(n), dim3(LB_FR_WG), LB_FR_EV_LDS, e->stream, d_coef, d_x,
                     d_scalars + (size_t)8 * (nb + n));
  LB_HIP(hipGetLastError());
  // 6. every ladder and subgroup check of the segment in one launch
  hipLaunchKernelGGL(k_g1_terms, dim3(nblk(n_pts)), dim3(LB_TPB), 0, e->stream, n_pts, d_pts, e->kzg.g1.as<uint32_t>(),
                     e->kzg.n, d_scalars, d_terms, d_term_status);
  LB_HIP(hipGetLastError());
  // 7. one wave per sidecar: status, T_k, the two-pair product
  hipLaunchKernelGGL(k_kzg_check_many, dim3(n), dim3(64), 0, e->stream, n, d_off, nb, d.status, d_pts, d_terms,
                     d_term_status, e->kzg.g2.as<uint32_t>(), d_ok);
  LB_HIP(hipGetLastError());
  // 8. the verdicts
  LB_HIP(hipMemcpyAsync(out_ok, d_ok, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// ---------------------------------------------------------------- KZG, one proof per blob (Deneb)
// compute_blob_kzg_proof for n_blobs blobs: every stage once over all of them, the 4096-term
// commitment to each quotient as in kzg_commit, one synchronisation at the end.
extern "C" int32_t lb_kzg_compute_blob_proofs(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs,
                                              const uint8_t* commitments48, uint8_t* out_proofs48, int32_t* out_status) {
  if (!kzg_ready(e) || n_blobs > kMaxBlobs) return LB_ERR_ARGUMENT;
  if (!n_blobs) return LB_OK;
  if (!blobs || !commitments48 || !out_proofs48 || !out_status) return LB_ERR_ARGUMENT;
  const uint32_t n = n_blobs;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, n);
  const kzg_lincomb_ws lin(w);
  uint32_t* d_coef = w.get<uint32_t>(n * kBlobBytes);
  uint32_t* d_quot_le = w.get<uint32_t>(n * kBlobBytes);
  uint8_t* d_commitments = w.get<uint8_t>((size_t)n * 48);
  uint32_t* d_units = w.get<uint32_t>((size_t)n * sizeof(fr));
  uint32_t* d_commit_terms = w.get<uint32_t>((size_t)n * sizeof(g1j));  // the validation launch's terms (unused)
  int32_t* d_commit_status = w.get<int32_t>((size_t)n * 4);
  uint32_t* d_z = w.get<uint32_t>((size_t)n * sizeof(fr));
  uint32_t* d_y = w.get<uint32_t>((size_t)n * sizeof(fr));
  uint8_t* d_proofs = w.get<uint8_t>((size_t)n * 48);
  LB_HIP(w.error());
  // 1. the blobs go up and are decoded; 2. the commitments are decoded and subgroup-checked (unit
  // scalars) while the host hashes the challenges
  LB_TRY(kzg_decode_async(e, d, n, blobs));
  std::vector<fr> ones(n), zs(n);
  for (uint32_t b = 0; b < n; b++) {
    ones[b] = fr_zero();
    ones[b].l[0] = 1;
  }
  LB_HIP(hipMemcpyAsync(d_commitments, commitments48, (size_t)n * 48, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_units, ones.data(), (size_t)n * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_g1_terms, dim3(nblk(n)), dim3(LB_TPB), 0, e->stream, n, d_commitments, e->kzg.g1.as<uint32_t>(),
                     e->kzg.n, d_units, d_commit_terms, d_commit_status);
  LB_HIP(hipGetLastError());
  kzg_blob_challenges(n, blobs, commitments48, zs.data(), kzg_hash_threads());
  LB_HIP(hipMemcpyAsync(d_z, zs.data(), (size_t)n * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  // 3. coefficients; 4. y_b and the quotients' scalars; 5. their commitments
  LB_TRY(kzg_intt(e, n, d.polys, d_coef, nullptr));
  hipLaunchKernelGGL(k_fr_eval_quotient_many, dim3(n), dim3(LB_FR_WG), LB_FR_EQ_LDS, e->stream, d_coef, d_z, d_quot_le, d_y);
  LB_HIP(hipGetLastError());
  LB_TRY(kzg_setup_lincombs(e, lin, n, d_quot_le, d_proofs));
  // 6. proofs and statuses: a commitment's rejection comes before its blob's
  std::vector<int32_t> blob_status(n, LB_OK), commit_status(n, LB_OK);
  LB_HIP(hipMemcpyAsync(out_proofs48, d_proofs, (size_t)n * 48, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(blob_status.data(), d.status, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(commit_status.data(), d_commit_status, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  kzg_fold_status(n, commit_status.data(), blob_status.data(), out_status, out_proofs48, 48);
  return LB_OK;
}

// verify_blob_kzg_proof_batch for many groups in one pass: every stage once over all blobs, two
// synchronisations (the combiner r_k hashes the y_i, which the device computes).  Device arrays in
// k_kzg_check_groups' order: the commitments, the proofs twice, one G1 generator per group.
extern "C" int32_t lb_kzg_verify_blob_proof_batch(lb_engine* e, uint32_t n_groups, const uint32_t* group_offsets,
                                                  const uint8_t* blobs, const uint8_t* commitments48,
                                                  const uint8_t* proofs48, int32_t* out_ok) {
  const uint32_t n = n_groups;
  if (!kzg_ready(e) || n > kMaxGroups) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  if (!out_ok || !kzg_offsets_ok(n, group_offsets, kMaxBlobs)) return LB_ERR_ARGUMENT;
  const uint32_t nb = group_offsets[n];
  if (nb && (!blobs || !commitments48 || !proofs48)) return LB_ERR_ARGUMENT;
  const uint32_t n_pts = 3 * nb + n;
  const size_t nb1 = std::max<size_t>(nb, 1);
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, nb1);
  uint32_t* d_off = w.get<uint32_t>((size_t)(n + 1) * 4);
  uint32_t* d_coef = w.get<uint32_t>(nb1 * kBlobBytes);
  uint32_t* d_z = w.get<uint32_t>(nb1 * sizeof(fr));
  uint32_t* d_y = w.get<uint32_t>(nb1 * sizeof(fr));
  uint8_t* d_pts = w.get<uint8_t>((size_t)n_pts * 48);
  uint32_t* d_scalars = w.get<uint32_t>((size_t)n_pts * 32);
  uint32_t* d_terms = w.get<uint32_t>((size_t)n_pts * sizeof(g1j));
  int32_t* d_term_status = w.get<int32_t>((size_t)n_pts * 4);
  int32_t* d_ok = w.get<int32_t>((size_t)n * 4);
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(d_off, group_offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
  // the host arrays live until the last synchronisation
  std::vector<fr> zs(nb1), ys(nb1), y_le(nb1), sc(n_pts);
  uint64_t hash_ns = 0;
  if (nb) {
    // 1. the blobs go up and are decoded while 2. the host threads hash the z_i
    LB_TRY(kzg_decode_async(e, d, nb, blobs));
    const auto t0 = kzg_clock::now();
    kzg_blob_challenges(nb, blobs, commitments48, zs.data(), kzg_hash_threads());
    hash_ns += kzg_ns_since(t0);
    // 3. coefficients, y_i = p_i(z_i), back to the host: the first synchronisation
    LB_HIP(hipMemcpyAsync(d_z, zs.data(), (size_t)nb * sizeof(fr), hipMemcpyHostToDevice, e->stream));
    LB_TRY(kzg_intt(e, nb, d.polys, d_coef, nullptr));
    hipLaunchKernelGGL(k_fr_eval_many, dim3(nb), dim3(LB_FR_WG), LB_FR_EV_LDS, e->stream, d_coef, d_z, d_y);
    LB_HIP(hipGetLastError());
    LB_HIP(hipMemcpyAsync(y_le.data(), d_y, (size_t)nb * sizeof(fr), hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    for (uint32_t j = 0; j < nb; j++) ys[j] = fr_to_mont(y_le[j]);
  }
  // 4. r_k per group and the scalars r^i, r^i z_i, sum r^i y_i
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t lo = group_offsets[k], cnt = group_offsets[k + 1] - lo;
    fr r = fr_one();
    if (cnt > 1) {  // r^0 = 1 alone is used otherwise: verify_blob_kzg_proof
      const auto t0 = kzg_clock::now();
      r = kzg_batch_r(cnt, commitments48 + (size_t)48 * lo, zs.data() + lo, ys.data() + lo, proofs48 + (size_t)48 * lo);
      hash_ns += kzg_ns_since(t0);
    }
    fr p = fr_one(), ysum = fr_zero();
    for (uint32_t i = 0; i < cnt; i++) {
      const uint32_t j = lo + i;
      fr_to_le_words(sc[j].l, p);
      fr_to_le_words(sc[nb + j].l, fr_mul(p, zs[j]));
      sc[2 * nb + j] = sc[j];
      ysum = fr_add(ysum, fr_mul(p, ys[j]));
      p = fr_mul(p, r);
    }
    fr_to_le_words(sc[3 * nb + k].l, ysum);
  }
  e->kzg.batch_hash_ns = hash_ns;
  std::vector<uint8_t> pts((size_t)n_pts * 48);
  if (nb) {
    memcpy(pts.data(), commitments48, (size_t)nb * 48);
    memcpy(pts.data() + (size_t)nb * 48, proofs48, (size_t)nb * 48);
    memcpy(pts.data() + (size_t)2 * nb * 48, proofs48, (size_t)nb * 48);
  }
  for (uint32_t k = 0; k < n; k++) memcpy(pts.data() + (size_t)(3 * nb + k) * 48, kG1Gen48, 48);
  LB_HIP(hipMemcpyAsync(d_scalars, sc.data(), (size_t)n_pts * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_pts, pts.data(), pts.size(), hipMemcpyHostToDevice, e->stream));
  // 5. every ladder and subgroup check of the call in one launch
  hipLaunchKernelGGL(k_g1_terms, dim3(nblk(n_pts)), dim3(LB_TPB), 0, e->stream, n_pts, d_pts, e->kzg.g1.as<uint32_t>(),
                     e->kzg.n, d_scalars, d_terms, d_term_status);
  LB_HIP(hipGetLastError());
  // 6. one wave per group: status, T_k and P_k, the two-pair product; the second synchronisation
  hipLaunchKernelGGL(k_kzg_check_groups, dim3(n), dim3(64), 0, e->stream, n, d_off, nb, d.status, d_terms, d_term_status,
                     e->kzg.g2.as<uint32_t>(), d_ok);
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(out_ok, d_ok, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

extern "C" uint64_t lb_kzg_batch_hash_ns(const lb_engine* e) { return e ? e->kzg.batch_hash_ns : 0; }

// ---------------------------------------------------------------- KZG cells (EIP-7594, PeerDAS)
// compute_cells for n_blobs blobs: decode, coefficients (k_fr_intt4096), then one workgroup per blob
// writes its 128 cells (k_fr_coset_ntt4096).
extern "C" int32_t lb_kzg_compute_cells(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out_cells,
                                        int32_t* out_status) {
  if (!kzg_ready(e) || n_blobs > kMaxBlobs) return LB_ERR_ARGUMENT;
  if (!n_blobs) return LB_OK;
  if (!blobs || !out_cells || !out_status) return LB_ERR_ARGUMENT;
  const uint32_t n = n_blobs;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, n);
  uint32_t* d_coef = w.get<uint32_t>(n * kBlobBytes);
  uint8_t* d_cells = w.get<uint8_t>(n * LB_FR_EXT_BYTES);
  LB_HIP(w.error());
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, n, blobs, blob_status));
  LB_TRY(kzg_intt(e, n, d.polys, d_coef, nullptr));
  LB_TRY(kzg_coset_ntt(e, n, d_coef, d.bytes, d_cells));
  LB_HIP(hipMemcpyAsync(out_cells, d_cells, n * LB_FR_EXT_BYTES, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  kzg_fold_status(n, blob_status.data(), nullptr, out_status, out_cells, LB_FR_EXT_BYTES);
  return LB_OK;
}

// The direct (non-FK20) proofs of chosen cells of one blob: the quotient by X^64 - h^64 per cell on
// the device (k_fr_cell_quotient), then one 4096-term linear combination of the setup per cell.
extern "C" int32_t lb_kzg_compute_cell_proofs(lb_engine* e, const uint8_t* blob, uint32_t n_cells, const uint32_t* cell_indices,
                                              uint8_t* out_proofs48, int32_t* out_status) {
  if (!kzg_ready(e) || !blob || !out_status || n_cells > LB_FR_CELLS) return LB_ERR_ARGUMENT;
  if (n_cells && (!cell_indices || !out_proofs48)) return LB_ERR_ARGUMENT;
  for (uint32_t c = 0; c < n_cells; c++)
    if (cell_indices[c] >= LB_FR_CELLS) return LB_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  const kzg_blobs d(w, 1);
  LB_HIP(w.error());
  std::vector<int32_t> blob_status;
  LB_TRY(kzg_load_blobs(e, d, 1, blob, blob_status));
  *out_status = blob_status[0];
  if (!n_cells) return LB_OK;
  if (*out_status != LB_OK) {
    memset(out_proofs48, 0, (size_t)n_cells * 48);
    return LB_OK;
  }
  const kzg_lincomb_ws lin(w);
  uint32_t* d_coef = w.get<uint32_t>(kBlobBytes);
  uint32_t* d_quot_le = w.get<uint32_t>(n_cells * kBlobBytes);
  uint32_t* d_cell_idx = w.get<uint32_t>((size_t)n_cells * 4);
  uint8_t* d_proofs = w.get<uint8_t>((size_t)n_cells * 48);
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(d_cell_idx, cell_indices, (size_t)n_cells * 4, hipMemcpyHostToDevice, e->stream));
  LB_TRY(kzg_intt(e, 1, d.polys, d_coef, nullptr));
  hipLaunchKernelGGL(k_fr_cell_quotient, dim3(n_cells), dim3(64), 0, e->stream, n_cells, d_coef, d_cell_idx,
                     e->kzg.cell_tab.as<uint32_t>(), d_quot_le);
  LB_HIP(hipGetLastError());
  LB_TRY(kzg_setup_lincombs(e, lin, n_cells, d_quot_le, d_proofs));
  LB_HIP(hipMemcpyAsync(out_proofs48, d_proofs, (size_t)n_cells * 48, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// verify_cell_kzg_proof_batch for many groups in one pass with ONE synchronisation: the combiner
// hashes only the caller's bytes, so every scalar of the given-point ladders is known on the host
// before anything comes back, and the interpolation coefficients never leave the device.
extern "C" int32_t lb_kzg_verify_cell_proof_batch(lb_engine* e, uint32_t n_groups, const uint32_t* cell_offsets,
                                                  const uint8_t* commitments48, const uint32_t* cell_indices,
                                                  const uint8_t* cells, const uint8_t* proofs48, int32_t* out_ok) {
  const uint32_t n = n_groups;
  if (!kzg_ready(e) || !e->kzg.cells || n > kMaxGroups) return LB_ERR_ARGUMENT;
  if (!n) return LB_OK;
  if (!out_ok || !kzg_offsets_ok(n, cell_offsets, kMaxCells)) return LB_ERR_ARGUMENT;
  const uint32_t nc = cell_offsets[n];
  if (nc && (!commitments48 || !cell_indices || !cells || !proofs48)) return LB_ERR_ARGUMENT;
  for (uint32_t k = 0; k < nc; k++)
    if (cell_indices[k] >= LB_FR_CELLS) return LB_ERR_ARGUMENT;
  const size_t nc1 = std::max<size_t>(nc, 1);
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  kzg_bufs w;
  uint8_t* d_cells = w.get<uint8_t>(nc1 * LB_FR_CELL_BYTES);
  uint32_t* d_cell_fr = w.get<uint32_t>(nc1 * LB_FR_CELL_BYTES);  // the cells as Montgomery Fr, then r^i I_k in place
  int32_t* d_cell_status = w.get<int32_t>(nc1 * 4);
  uint32_t* d_cell_idx = w.get<uint32_t>(nc1 * 4);
  uint32_t* d_weights = w.get<uint32_t>(nc1 * sizeof(fr));
  uint32_t* d_off = w.get<uint32_t>((size_t)(n + 1) * 4);
  uint32_t* d_doff = w.get<uint32_t>((size_t)(n + 1) * 4);
  uint32_t* d_tab_scalars = w.get<uint32_t>((size_t)n * 64 * sizeof(fr));
  int32_t* d_ok = w.get<int32_t>((size_t)n * 4);
  LB_HIP(w.error());
  // 1. the cells go up and are decoded (kzg_decode_async's stanza over k_fr_cell_load, the cell
  // indices going up inside it) while 2. the host deduplicates and hashes
  LB_HIP(hipMemcpyAsync(d_off, cell_offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
  if (nc) {
    LB_HIP(hipMemcpyAsync(d_cells, cells, (size_t)nc * LB_FR_CELL_BYTES, hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipMemcpyAsync(d_cell_idx, cell_indices, (size_t)nc * 4, hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipMemsetAsync(d_cell_status, 0, (size_t)nc * 4, e->stream));
    const uint32_t n_elems = nc * LB_FR_CELL;
    hipLaunchKernelGGL(k_fr_cell_load, dim3((n_elems + 255) / 256), dim3(256), 0, e->stream, n_elems, d_cells, d_cell_fr,
                       d_cell_status);
    LB_HIP(hipGetLastError());
  }
  // the host arrays live until the synchronisation
  std::vector<uint32_t> ci(nc1), first, doff(n + 1, 0);
  std::vector<fr> rs(n), wt(nc1);
  const auto t0 = kzg_clock::now();
  for (uint32_t g = 0; g < n; g++) {
    const uint32_t lo = cell_offsets[g];
    doff[g + 1] = doff[g] + kzg_cell_dedup(cell_offsets[g + 1] - lo, commitments48 + (size_t)48 * lo, ci.data() + lo, first);
  }
  kzg_cell_batch_rs(n, cell_offsets, doff.data(), commitments48, ci.data(), first.data(), cell_indices, cells, proofs48,
                    rs.data(), kzg_hash_threads());
  e->kzg.batch_hash_ns = kzg_ns_since(t0);
  // 3. the scalars: r^i per proof, r^i h^64 per proof, the summed r^i per distinct commitment
  const uint32_t nd = doff[n], n_pts = 2 * nc + nd;
  const size_t np1 = std::max<size_t>(n_pts, 1);
  std::vector<fr> sc(np1);
  std::vector<uint8_t> pts(np1 * 48);
  for (uint32_t g = 0; g < n; g++) {
    const uint32_t lo = cell_offsets[g], cnt = cell_offsets[g + 1] - lo, dcnt = doff[g + 1] - doff[g];
    std::vector<fr> wsum(dcnt, fr_zero());
    fr p = fr_one();
    for (uint32_t i = 0; i < cnt; i++) {
      const uint32_t k = lo + i;
      wt[k] = p;
      fr_to_le_words(sc[k].l, p);
      fr_to_le_words(sc[nc + k].l, fr_mul(p, e->kzg.h64[cell_indices[k]]));
      wsum[ci[k]] = fr_add(wsum[ci[k]], p);
      p = fr_mul(p, rs[g]);
    }
    for (uint32_t j = 0; j < dcnt; j++) {
      fr_to_le_words(sc[2 * nc + doff[g] + j].l, wsum[j]);
      memcpy(pts.data() + (size_t)(2 * nc + doff[g] + j) * 48, commitments48 + (size_t)48 * (lo + first[doff[g] + j]), 48);
    }
  }
  if (nc) {
    memcpy(pts.data(), proofs48, (size_t)nc * 48);
    memcpy(pts.data() + (size_t)nc * 48, proofs48, (size_t)nc * 48);
  }
  const uint32_t n_tab = n * LB_FR_CELL, n_terms = n_pts + n_tab;
  uint8_t* d_pts = w.get<uint8_t>(np1 * 48);
  uint32_t* d_scalars = w.get<uint32_t>(np1 * 32);
  uint32_t* d_terms = w.get<uint32_t>((size_t)n_terms * sizeof(g1j));
  int32_t* d_term_status = w.get<int32_t>((size_t)n_terms * 4);
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(d_doff, doff.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
  if (nc) {
    LB_HIP(hipMemcpyAsync(d_weights, wt.data(), (size_t)nc * sizeof(fr), hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipMemcpyAsync(d_scalars, sc.data(), (size_t)n_pts * sizeof(fr), hipMemcpyHostToDevice, e->stream));
    LB_HIP(hipMemcpyAsync(d_pts, pts.data(), (size_t)n_pts * 48, hipMemcpyHostToDevice, e->stream));
    // 4. one wave per cell: r^i I_k, in place; then 5. the per-group sums, negated, as scalars
    hipLaunchKernelGGL(k_fr_cell_interp, dim3(nc), dim3(64), 0, e->stream, nc, d_cell_fr, d_cell_idx, d_weights,
                       e->kzg.cell_tab.as<uint32_t>());
    LB_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_fr_cell_sum, dim3(n), dim3(64), 0, e->stream, n, d_off, nc, d_cell_fr, d_tab_scalars);
  LB_HIP(hipGetLastError());
  // 6. every ladder of the call in one launch: the given points and the 64 setup points per group
  hipLaunchKernelGGL(k_g1_cell_terms, dim3(nblk(n_terms)), dim3(LB_TPB), 0, e->stream, n_pts, d_pts, d_scalars, n_tab,
                     e->kzg.g1.as<uint32_t>(), e->kzg.n, (uint32_t)LB_FR_CELL, d_tab_scalars, d_terms, d_term_status);
  LB_HIP(hipGetLastError());
  // 7. one wave per group: status, LL and RL, the two-pair product; the synchronisation
  hipLaunchKernelGGL(k_kzg_check_cells, dim3(n), dim3(64), 0, e->stream, n, d_off, nc, d_doff, nd, d_cell_status, d_terms,
                     d_term_status, e->kzg.g2.as<uint32_t>(), d_ok);
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(out_ok, d_ok, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// ---------------------------------------------------------------- KZG cells and all their proofs (FK20; lb_fk20.h)
namespace {
// n_tr transforms of 128 points between g1j SoA buffers (k_g1_fft128); tw_entry: LB_FK_TAB_FWD / _INV
void kzg_fk_fft(lb_engine* e, uint32_t n_tr, const uint32_t* in, uint32_t in_cap, uint32_t in_st, uint32_t in_sj, uint32_t n_live,
                uint32_t tw_entry, uint32_t* out, uint32_t out_cap, uint32_t out_st, uint32_t out_sm) {
  hipLaunchKernelGGL(k_g1_fft128, dim3(n_tr), dim3(64), 0, e->stream, n_tr, in, in_cap, in_st, in_sj, n_live,
                     e->kzg.fk_tw.as<uint32_t>() + (size_t)8 * tw_entry, (const uint32_t*)nullptr, out, out_cap, out_st, out_sm);
}

// The extended setup X_i[r] = DFT128(x_i)[r] at entry 64 r + i, once per loaded setup: the 64 strided,
// padded columns of the setup (k_g1_fk_gather), one transform each.  Caller holds e->mu.
int32_t kzg_fk_table(lb_engine* e) {
  kzg_state& kz = e->kzg;
  if (kz.fk_ready) return LB_OK;
  std::vector<fr> tab(LB_FK_TAB_LEN);
  fk_tables(tab.data());
  kzg_bufs w;
  LB_HIP(kz.fk_tw.ensure(tab.size() * sizeof(fr)));
  LB_HIP(kz.fk_x.ensure((size_t)LB_FK_POINTS * sizeof(g1j)));
  uint32_t* d_columns = w.get<uint32_t>((size_t)LB_FK_POINTS * sizeof(g1j));  // the gathered columns
  LB_HIP(w.error());
  LB_HIP(hipMemcpyAsync(kz.fk_tw.p, tab.data(), tab.size() * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_g1_fk_gather, dim3(nblk(LB_FK_POINTS)), dim3(LB_TPB), 0, e->stream, kz.g1.as<uint32_t>(), kz.n,
                     d_columns);
  kzg_fk_fft(e, LB_FK_COLS, d_columns, LB_FK_POINTS, LB_FK_N, 1, LB_FK_N, LB_FK_TAB_FWD, kz.fk_x.as<uint32_t>(), LB_FK_POINTS, 1,
             LB_FK_COLS);
  LB_HIP(hipGetLastError());
  LB_HIP(hipStreamSynchronize(e->stream));
  kz.fk_ready = true;
  return LB_OK;
}
}  // namespace

namespace {
// The device buffers of FK20's steps 2 - 4 for n blobs, and those steps: from the blobs' Montgomery
// coefficients (d_coef) to their 128 compressed proofs each (d_proofs).  Shared by
// lb_kzg_compute_cells_and_proofs and lb_kzg_recover_cells_and_proofs.  Does not synchronise.
struct kzg_fk_ws {
  uint32_t* col_scalars;
  uint32_t* terms;
  uint32_t* sums;  // E[r], then the proofs as Jacobian points
  uint32_t* h;
  uint8_t* proofs;
  kzg_fk_ws(kzg_bufs& w, size_t n)
      : col_scalars(w.get<uint32_t>(n * LB_FK_POINTS * sizeof(fr))), terms(w.get<uint32_t>(n * LB_FK_POINTS * sizeof(g1j))),
        sums(w.get<uint32_t>(n * LB_FK_N * sizeof(g1j))), h(w.get<uint32_t>(n * LB_FK_N * sizeof(g1j))),
        proofs(w.get<uint8_t>(n * LB_FK_N * 48)) {}
};
int32_t kzg_fk_proofs(lb_engine* e, const kzg_fk_ws& f, uint32_t n, const uint32_t* d_coef) {
  const uint32_t np = n * LB_FK_N, nt = n * LB_FK_POINTS;
  // 2. the 64 column transforms per blob -> the scalars C_i[r] / 128 in the table's order
  hipLaunchKernelGGL(k_fr_fk_cols, dim3(n * LB_FK_COLS), dim3(64), 0, e->stream, n, d_coef, e->kzg.fk_tw.as<uint32_t>(),
                     f.col_scalars);
  // 3. every ladder of the call in one launch, then E[r]: entry 128 b + r of f.sums
  hipLaunchKernelGGL(k_g1_jac_terms, dim3(nblk(nt)), dim3(LB_TPB), 0, e->stream, nt, e->kzg.fk_x.as<uint32_t>(), LB_FK_POINTS,
                     f.col_scalars, f.terms);
  hipLaunchKernelGGL(k_g1_sum64, dim3(np), dim3(64), 0, e->stream, nt, f.terms, np, f.sums);
  LB_HIP(hipGetLastError());
  // 4. h = IDFT(E) (scaled already); the proofs = DFT(h[0 .. 63], O ...): h[64 .. 127] are dropped by the load
  kzg_fk_fft(e, n, f.sums, np, LB_FK_N, 1, LB_FK_N, LB_FK_TAB_INV, f.h, np, LB_FK_N, 1);
  kzg_fk_fft(e, n, f.h, np, LB_FK_N, 1, LB_FK_LIVE, LB_FK_TAB_FWD, f.sums, np, LB_FK_N, 1);
  hipLaunchKernelGGL(k_g1_fk_out48, dim3(np / 64), dim3(64), 0, e->stream, np, f.sums, f.proofs);
  LB_HIP(hipGetLastError());
  return LB_OK;
}
}  // namespace

// compute_cells_and_kzg_proofs for n_blobs blobs with ONE synchronisation (after the table's first
// build): a blob with an element >= r still runs, on the reduced element, and is zeroed afterwards.
extern "C" int32_t lb_kzg_compute_cells_and_proofs(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out_cells,
                                                   uint8_t* out_proofs48, int32_t* out_status) {
  if (!kzg_ready(e) || n_blobs > kMaxFkBlobs) return LB_ERR_ARGUMENT;
  if (!n_blobs) return LB_OK;
  if (!blobs || !out_cells || !out_proofs48 || !out_status) return LB_ERR_ARGUMENT;
  const uint32_t n = n_blobs;
  const size_t proof_bytes = (size_t)LB_FK_N * 48;
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  LB_TRY(kzg_fk_table(e));
  kzg_bufs w;
  const kzg_blobs d(w, n);
  uint32_t* d_coef = w.get<uint32_t>(n * kBlobBytes);
  uint8_t* d_cells = w.get<uint8_t>(n * LB_FR_EXT_BYTES);
  const kzg_fk_ws fk(w, n);
  LB_HIP(w.error());
  // 1. decode, coefficients, and the cells by the path of lb_kzg_compute_cells
  LB_TRY(kzg_decode_async(e, d, n, blobs));
  LB_TRY(kzg_intt(e, n, d.polys, d_coef, nullptr));
  LB_TRY(kzg_coset_ntt(e, n, d_coef, d.bytes, d_cells));
  // 2. - 4. FK20 from the coefficients
  LB_TRY(kzg_fk_proofs(e, fk, n, d_coef));
  std::vector<int32_t> blob_status(n, LB_OK);
  LB_HIP(hipMemcpyAsync(out_cells, d_cells, n * LB_FR_EXT_BYTES, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(out_proofs48, fk.proofs, n * proof_bytes, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(blob_status.data(), d.status, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  kzg_fold_status(n, blob_status.data(), nullptr, out_status, out_cells, LB_FR_EXT_BYTES, out_proofs48, proof_bytes);
  return LB_OK;
}

// recover_cells_and_kzg_proofs for n_blobs blobs with ONE synchronisation (after the table's first
// build).  The host validates the indices and builds each blob's present-cell mask; everything else
// is on the device: decode (k_fr_cell_load), the cells' interpolation polynomials (k_fr_cell_interp,
// unit weights), the erasure decode (lb_recover.h: k_fr_recover_zero, k_fr_recover_cols) into the
// blobs' coefficients, then every cell from those coefficients (k_fr_ntt4096, k_fr_coset_ntt4096)
// and FK20.  A blob with an element >= r or with inconsistent cells still runs and is zeroed afterwards.
extern "C" int32_t lb_kzg_recover_cells_and_proofs(lb_engine* e, uint32_t n_blobs, const uint32_t* cell_offsets,
                                                   const uint32_t* cell_indices, const uint8_t* cells, uint8_t* out_cells,
                                                   uint8_t* out_proofs48, int32_t* out_status) {
  if (!kzg_ready(e) || n_blobs > kMaxFkBlobs) return LB_ERR_ARGUMENT;
  if (!n_blobs) return LB_OK;
  if (!cell_offsets || !cell_indices || !cells || !out_cells || !out_proofs48 || !out_status) return LB_ERR_ARGUMENT;
  const uint32_t n = n_blobs;
  std::vector<uint32_t> mask((size_t)n * LB_RC_MASK_WORDS, 0);
  if (!kzg_recover_plan(n, cell_offsets, cell_indices, mask.data())) return LB_ERR_ARGUMENT;
  const uint32_t nc = cell_offsets[n];
  const size_t proof_bytes = (size_t)LB_FK_N * 48;
  std::vector<fr> ones(nc, fr_one());  // the host arrays live until the synchronisation
  std::lock_guard<std::mutex> lk(e->mu);
  LB_HIP(hipSetDevice(e->device));
  LB_TRY(kzg_fk_table(e));
  kzg_bufs w;
  uint8_t* d_in = w.get<uint8_t>((size_t)nc * LB_FR_CELL_BYTES);
  uint32_t* d_cell_fr = w.get<uint32_t>((size_t)nc * LB_FR_CELL_BYTES);  // the cells as Montgomery Fr, then I_k in place
  int32_t* d_cell_status = w.get<int32_t>((size_t)nc * 4);
  uint32_t* d_cell_idx = w.get<uint32_t>((size_t)nc * 4);
  uint32_t* d_weights = w.get<uint32_t>((size_t)nc * sizeof(fr));
  uint32_t* d_off = w.get<uint32_t>((size_t)(n + 1) * 4);
  uint32_t* d_mask = w.get<uint32_t>(mask.size() * 4);
  uint32_t* d_zev = w.get<uint32_t>((size_t)n * LB_FK_N * sizeof(fr));
  uint32_t* d_zcinv = w.get<uint32_t>((size_t)n * LB_FK_N * sizeof(fr));
  int32_t* d_fit_status = w.get<int32_t>((size_t)n * 4);
  uint32_t* d_coef = w.get<uint32_t>(n * kBlobBytes);
  uint8_t* d_blob_bytes = w.get<uint8_t>(n * kBlobBytes);
  uint8_t* d_cells = w.get<uint8_t>(n * LB_FR_EXT_BYTES);
  const kzg_fk_ws fk(w, n);
  LB_HIP(w.error());
  // 1. the cells go up and are decoded; 2. their interpolation polynomials, in place
  LB_HIP(hipMemcpyAsync(d_in, cells, (size_t)nc * LB_FR_CELL_BYTES, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_cell_idx, cell_indices, (size_t)nc * 4, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_weights, ones.data(), (size_t)nc * sizeof(fr), hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_off, cell_offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemcpyAsync(d_mask, mask.data(), mask.size() * 4, hipMemcpyHostToDevice, e->stream));
  LB_HIP(hipMemsetAsync(d_cell_status, 0, (size_t)nc * 4, e->stream));
  LB_HIP(hipMemsetAsync(d_fit_status, 0, (size_t)n * 4, e->stream));
  const uint32_t n_elems = nc * LB_FR_CELL;
  hipLaunchKernelGGL(k_fr_cell_load, dim3((n_elems + 255) / 256), dim3(256), 0, e->stream, n_elems, d_in, d_cell_fr, d_cell_status);
  hipLaunchKernelGGL(k_fr_cell_interp, dim3(nc), dim3(64), 0, e->stream, nc, d_cell_fr, d_cell_idx, d_weights,
                     e->kzg.cell_tab.as<uint32_t>());
  LB_HIP(hipGetLastError());
  // 3. per blob the vanishing polynomial's values, per (blob, column) the decode -> the coefficients
  hipLaunchKernelGGL(k_fr_recover_zero, dim3(n), dim3(64), 0, e->stream, n, d_mask, e->kzg.fk_tw.as<uint32_t>(),
                     e->kzg.cell_tab.as<uint32_t>(), d_zev, d_zcinv);
  hipLaunchKernelGGL(k_fr_recover_cols, dim3(n * LB_FK_COLS), dim3(64), 0, e->stream, n, d_cell_fr, nc, d_off, d_mask, d_zev, d_zcinv,
                     e->kzg.fk_tw.as<uint32_t>(), e->kzg.cell_tab.as<uint32_t>(), d_coef, d_fit_status);
  LB_HIP(hipGetLastError());
  // 4. every cell from the coefficients: the blob's bytes, then the path of lb_kzg_compute_cells
  LB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fr_ntt4096), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)LB_FR_INTT_LDS));
  hipLaunchKernelGGL(k_fr_ntt4096, dim3(n), dim3(LB_FR_WG), LB_FR_INTT_LDS, e->stream, d_coef, e->kzg.cell_tab.as<uint32_t>(),
                     d_blob_bytes);
  LB_HIP(hipGetLastError());
  LB_TRY(kzg_coset_ntt(e, n, d_coef, d_blob_bytes, d_cells));
  // 5. FK20 from the coefficients
  LB_TRY(kzg_fk_proofs(e, fk, n, d_coef));
  std::vector<int32_t> cell_status(nc, LB_OK), scalar_status(n, LB_OK), fit_status(n, LB_OK);
  LB_HIP(hipMemcpyAsync(out_cells, d_cells, n * LB_FR_EXT_BYTES, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(out_proofs48, fk.proofs, n * proof_bytes, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(cell_status.data(), d_cell_status, (size_t)nc * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipMemcpyAsync(fit_status.data(), d_fit_status, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  // an element >= r comes before the cells' inconsistency
  for (uint32_t b = 0; b < n; b++)
    for (uint32_t k = cell_offsets[b]; k < cell_offsets[b + 1]; k++)
      if (cell_status[k] != LB_OK) scalar_status[b] = LB_BAD_SCALAR;
  kzg_fold_status(n, scalar_status.data(), fit_status.data(), out_status, out_cells, LB_FR_EXT_BYTES, out_proofs48, proof_bytes);
  return LB_OK;
}
