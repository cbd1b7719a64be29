// The Fiat-Shamir transcripts of the KZG calls, hashed on the host (host-only: lb_engine.hip's host
// pass and the CPU harness include it; no kernel does).  sha_stream is the streaming SHA-256 every
// transcript goes through; kzg_blob_challenge and kzg_batch_r are the two transcripts of the
// per-blob (Deneb) proof form, restated in lodestar_amd/kzg.py compute_challenge / compute_batch_r:
//   z_i = hash_to_bls_field(FS_DOMAIN || 4096 as 16 bytes BE || blob_i || C_i)
//   r   = hash_to_bls_field(RC_DOMAIN || 4096 as 8 bytes BE || n as 8 bytes BE ||
//                           for each i: C_i || z_i (32 BE) || y_i (32 BE) || proof_i)
// with hash_to_bls_field = SHA-256 read as a big-endian integer mod r (no tag byte, unlike the
// aggregate form's transcript in lb_engine.hip).
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
