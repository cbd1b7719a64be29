// The Fiat-Shamir transcripts of the KZG calls, hashed on the host (host-only: lb_kzg_host.hip's host
// pass and the CPU harness include it; no kernel does).  sha_stream is the streaming SHA-256 every
// transcript goes through; kzg_blob_challenge and kzg_batch_r are the two transcripts of the
// per-blob (Deneb) proof form, restated in lodestar_amd/kzg.py compute_challenge / compute_batch_r:
//   z_i = hash_to_bls_field(FS_DOMAIN || 4096 as 16 bytes BE || blob_i || C_i)
//   r   = hash_to_bls_field(RC_DOMAIN || 4096 as 8 bytes BE || n as 8 bytes BE ||
//                           for each i: C_i || z_i (32 BE) || y_i (32 BE) || proof_i)
// with hash_to_bls_field = SHA-256 read as a big-endian integer mod r (no tag byte, unlike the
// aggregate form's transcript in lb_kzg_host.hip).
#pragma once
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>
#include "lb_fr.h"
#include "lb_h2c.h"

// SHA-256 of the Fiat-Shamir transcript, streamed through lb_h2c.h's sha256_compress on the host
struct sha_stream {
  uint32_t h[8];
  uint8_t buf[64];
  size_t fill = 0;
  uint64_t total = 0;
  sha_stream() { sha256_init(h); }
  void block(const uint8_t* b) {
    uint32_t w[16];
    for (int i = 0; i < 16; i++)
      w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
    sha256_compress(h, w);
  }
  void update(const uint8_t* d, size_t n) {
    total += n;
    if (fill) {
      const size_t k = std::min(n, sizeof(buf) - fill);
      memcpy(buf + fill, d, k);
      fill += k;
      d += k;
      n -= k;
      if (fill < sizeof(buf)) return;
      block(buf);
      fill = 0;
    }
    for (; n >= 64; d += 64, n -= 64) block(d);
    if (n) memcpy(buf, d, n);
    fill = n;
  }
  void finish(uint8_t out[32]) {
    const uint64_t bits = total * 8;
    uint8_t pad[72] = {0x80};
    const size_t padn = (fill < 56 ? 56 : 120) - fill;
    uint8_t len[8];
    for (int i = 0; i < 8; i++) len[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(pad, padn);
    update(len, 8);
    for (int i = 0; i < 8; i++)
      for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
  }
};

#define LB_KZG_BLOB_ELEMS 4096u  // FIELD_ELEMENTS_PER_BLOB (LB_FR_N of lb_kzg_field.h)
#define LB_KZG_BLOB_BYTES ((size_t)LB_KZG_BLOB_ELEMS * 32)

// a finished digest as a field element (Montgomery form): big-endian integer mod r
static inline fr kzg_digest_to_field(sha_stream& s) {
  uint8_t d[32];
  s.finish(d);
  uint32_t w[8];
  for (int k = 0; k < 8; k++)
    w[k] = ((uint32_t)d[28 - 4 * k] << 24) | ((uint32_t)d[29 - 4 * k] << 16) | ((uint32_t)d[30 - 4 * k] << 8) | d[31 - 4 * k];
  return fr_reduce256(w);
}
// a field element (Montgomery form) as 32 big-endian bytes
static inline void kzg_fr_to_be32(uint8_t out[32], const fr& a) {
  uint32_t w[8];
  fr_to_le_words(w, a);
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) out[31 - 4 * k - s] = (uint8_t)(w[k] >> (8 * s));
}

// compute_challenge: the evaluation point of one blob and its commitment
static inline fr kzg_blob_challenge(const uint8_t* blob, const uint8_t* commitment48) {
  sha_stream s;
  s.update(reinterpret_cast<const uint8_t*>("FSBLOBVERIFY_V1_"), 16);
  uint8_t be[16] = {0};
  be[14] = (uint8_t)(LB_KZG_BLOB_ELEMS >> 8);
  be[15] = (uint8_t)LB_KZG_BLOB_ELEMS;
  s.update(be, 16);
  s.update(blob, LB_KZG_BLOB_BYTES);
  s.update(commitment48, 48);
  return kzg_digest_to_field(s);
}

// the random combiner of one verify_blob_kzg_proof_batch call over n (C_i, z_i, y_i, proof_i)
static inline fr kzg_batch_r(uint32_t n, const uint8_t* commitments48, const fr* z, const fr* y, const uint8_t* proofs48) {
  sha_stream s;
  s.update(reinterpret_cast<const uint8_t*>("RCKZGBATCH___V1_"), 16);
  uint8_t be[16] = {0};
  be[6] = (uint8_t)(LB_KZG_BLOB_ELEMS >> 8);
  be[7] = (uint8_t)LB_KZG_BLOB_ELEMS;
  for (int i = 0; i < 4; i++) be[12 + i] = (uint8_t)(n >> (24 - 8 * i));
  s.update(be, 16);
  for (uint32_t i = 0; i < n; i++) {
    uint8_t zy[64];
    kzg_fr_to_be32(zy, z[i]);
    kzg_fr_to_be32(zy + 32, y[i]);
    s.update(commitments48 + (size_t)48 * i, 48);
    s.update(zy, 64);
    s.update(proofs48 + (size_t)48 * i, 48);
  }
  return kzg_digest_to_field(s);
}

// ------------------------------------------------------------------ cell batches (EIP-7594)
// verify_cell_kzg_proof_batch, restated in lodestar_amd/kzg.py compute_cell_batch_r: the commitments
// of one call are deduplicated in order of first appearance, and
//   r = hash_to_bls_field(CELL_DOMAIN || 4096 || 64 || #distinct commitments || n ||
//                         every distinct commitment ||
//                         for each cell k: commitment_indices[k] || cell_indices[k] || cell_k || proof_k)
// with every integer as 8 bytes BE and a cell as its 64 elements, 32 bytes BE each (its own bytes).
// Nothing the device computes enters it.
#define LB_KZG_CELL_BYTES 2048u  // BYTES_PER_CELL

// Deduplicate the n commitments (48 bytes each) of one group: ci[k] = the index of cell k's
// commitment among the distinct ones, first[d] = the position where distinct commitment d first
// appears (appended to `first`).  Returns the number of distinct commitments.
static inline uint32_t kzg_cell_dedup(uint32_t n, const uint8_t* commitments48, uint32_t* ci, std::vector<uint32_t>& first) {
  std::vector<uint32_t> order(n);
  for (uint32_t k = 0; k < n; k++) order[k] = k;
  // equal byte strings side by side, the earliest position first within each run
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int c = memcmp(commitments48 + (size_t)48 * a, commitments48 + (size_t)48 * b, 48);
    return c != 0 ? c < 0 : a < b;
  });
  std::vector<uint32_t> rep(n);  // rep[k]: the first position with cell k's commitment
  for (uint32_t i = 0; i < n; i++) {
    const bool same = i > 0 && memcmp(commitments48 + (size_t)48 * order[i], commitments48 + (size_t)48 * order[i - 1], 48) == 0;
    rep[order[i]] = same ? rep[order[i - 1]] : order[i];
  }
  const size_t base = first.size();
  for (uint32_t k = 0; k < n; k++) {
    if (rep[k] == k) {
      ci[k] = (uint32_t)(first.size() - base);
      first.push_back(k);
    } else {
      ci[k] = ci[rep[k]];
    }
  }
  return (uint32_t)(first.size() - base);
}

static inline void kzg_be64(uint8_t out[8], uint64_t v) {
  for (int i = 0; i < 8; i++) out[i] = (uint8_t)(v >> (56 - 8 * i));
}

// the combiner of one group of n cells; ci / first (n_distinct entries) from kzg_cell_dedup
static inline fr kzg_cell_batch_r(uint32_t n, const uint8_t* commitments48, const uint32_t* ci, const uint32_t* first,
                                  uint32_t n_distinct, const uint32_t* cell_indices, const uint8_t* cells,
                                  const uint8_t* proofs48) {
  sha_stream s;
  s.update(reinterpret_cast<const uint8_t*>("RCKZGCBATCH__V1_"), 16);
  uint8_t be[32];
  kzg_be64(be, LB_KZG_BLOB_ELEMS);
  kzg_be64(be + 8, LB_KZG_CELL_BYTES / 32);
  kzg_be64(be + 16, n_distinct);
  kzg_be64(be + 24, n);
  s.update(be, 32);
  for (uint32_t d = 0; d < n_distinct; d++) s.update(commitments48 + (size_t)48 * first[d], 48);
  for (uint32_t k = 0; k < n; k++) {
    kzg_be64(be, ci[k]);
    kzg_be64(be + 8, cell_indices[k]);
    s.update(be, 16);
    s.update(cells + (size_t)LB_KZG_CELL_BYTES * k, LB_KZG_CELL_BYTES);
    s.update(proofs48 + (size_t)48 * k, 48);
  }
  return kzg_digest_to_field(s);
}

// r_g for n_groups groups on `threads` host threads (group g on thread g mod threads), all joined
// before this returns.  Group g owns cells off[g] .. off[g + 1] - 1 of the flat per-cell arrays and
// the distinct commitments doff[g] .. doff[g + 1] - 1 of `first` (positions within the group).
static inline void kzg_cell_batch_rs(uint32_t n_groups, const uint32_t* off, const uint32_t* doff, const uint8_t* commitments48,
                                     const uint32_t* ci, const uint32_t* first, const uint32_t* cell_indices,
                                     const uint8_t* cells, const uint8_t* proofs48, fr* r, uint32_t threads) {
  threads = std::max(1u, std::min(threads, n_groups));
  auto work = [=](uint32_t t) {
    for (uint32_t g = t; g < n_groups; g += threads) {
      const uint32_t lo = off[g];
      r[g] = kzg_cell_batch_r(off[g + 1] - lo, commitments48 + (size_t)48 * lo, ci + lo, first + doff[g], doff[g + 1] - doff[g],
                              cell_indices + lo, cells + (size_t)LB_KZG_CELL_BYTES * lo, proofs48 + (size_t)48 * lo);
    }
  };
  if (threads == 1) {
    work(0);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve(threads - 1);
  for (uint32_t t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (std::thread& th : pool) th.join();
}

// z_i for n blobs on `threads` host threads (blob i on thread i mod threads), all joined before
// this returns; one thread hashes in the caller's own
static inline void kzg_blob_challenges(uint32_t n, const uint8_t* blobs, const uint8_t* commitments48, fr* z,
                                       uint32_t threads) {
  threads = std::max(1u, std::min(threads, n));
  auto work = [=](uint32_t t) {
    for (uint32_t i = t; i < n; i += threads) z[i] = kzg_blob_challenge(blobs + i * LB_KZG_BLOB_BYTES, commitments48 + (size_t)48 * i);
  };
  if (threads == 1) {
    work(0);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve(threads - 1);
  for (uint32_t t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (std::thread& th : pool) th.join();
}
