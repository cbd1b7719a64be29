// The parts of the KZG calls' host code (lb_kzg_host.hip) that touch no device: the per-call caps,
// the offsets validator, the status fold and the little-endian scalar reader.  Host-only; the CPU
// harness includes it too (tests/test_kzg_blob_cpu.py).
#pragma once
#include <string.h>
#include "lb_fr.h"

constexpr uint32_t kMaxBlobs = 1024;    // blobs per call (the spec's MAX_BLOBS_PER_BLOCK is 4)
constexpr uint32_t kMaxFkBlobs = 128;   // ... per FK20 call: 8192 ladders and 1.2 MB of terms per blob
constexpr uint32_t kMaxGroups = 1024;   // sidecars or groups per batched verification
constexpr uint32_t kMaxCells = 16384;   // cells per lb_kzg_verify_cell_proof_batch call

// off[0 .. n] splits a flat array into n groups: starts at 0, never decreases, ends at or below cap
static inline bool kzg_offsets_ok(uint32_t n, const uint32_t* off, uint32_t cap) {
  if (!off || off[0] != 0) return false;
  for (uint32_t k = 0; k < n; k++)
    if (off[k + 1] < off[k]) return false;
  return off[n] <= cap;
}

// out_status[i] = first[i] if that rejects item i, else second[i] (second may be null: LB_OK); a
// rejected item's outputs (stride0 bytes of out0 and, if given, stride1 bytes of out1) are zeroed
static inline void kzg_fold_status(uint32_t n, const int32_t* first, const int32_t* second, int32_t* out_status,
                                   uint8_t* out0, size_t stride0, uint8_t* out1 = nullptr, size_t stride1 = 0) {
  for (uint32_t i = 0; i < n; i++) {
    out_status[i] = first[i] != LB_OK ? first[i] : (second ? second[i] : LB_OK);
    if (out_status[i] == LB_OK) continue;
    memset(out0 + i * stride0, 0, stride0);
    if (out1) memset(out1 + i * stride1, 0, stride1);
  }
}

// lb_kzg_recover_cells_and_proofs' argument check: off[0 .. n] splits idx into n blobs' given cells,
// each blob has 64 .. 128 of them, every index is below 128 and a blob's indices strictly ascend (the
// spec's sorted and no-duplicates checks).  mask: 4 words per blob, zeroed by the caller; bit
// (i mod 32) of word 4 b + i div 32 is set where blob b's cell i is given (lb_recover.h rc_present).
static inline bool kzg_recover_plan(uint32_t n, const uint32_t* off, const uint32_t* idx, uint32_t* mask) {
  if (!kzg_offsets_ok(n, off, n * 128u)) return false;
  for (uint32_t b = 0; b < n; b++) {
    const uint32_t lo = off[b], cnt = off[b + 1] - lo;
    if (cnt < 64u || cnt > 128u) return false;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t i = idx[lo + k];
      if (i >= 128u || (k && i <= idx[lo + k - 1])) return false;
      mask[4 * b + (i >> 5)] |= 1u << (i & 31u);
    }
  }
  return true;
}

// 32 little-endian bytes as a field element's words: plain form, not range-checked (fr_lt_mod)
static inline fr kzg_fr_from_le32(const uint8_t* b) {
  fr a;
  for (int k = 0; k < 8; k++)
    a.l[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
  return a;
}
