// CPU harness of the host and per-lane pieces of the per-blob (Deneb) KZG calls: the two transcripts
// of lb_kzg_transcript.h (kzg_blob_challenge, kzg_batch_r, the threaded kzg_blob_challenges), the
// phases of k_fr_eval_quotient_many (kzg_blob_lanes.h over lb_fr.h fr_eq_*) and the status fold of
// k_kzg_check_groups (lb_fr.h kzg_group_status), and the device-free helpers of the calls' host code
// (lb_kzg_host.h: the offsets validator, the per-item status fold), compiled as plain C++ for
// tests/test_kzg_blob_cpu.py.  Field elements cross the boundary as 32 bytes: big endian where the
// transcript has them so, little endian plain form for the scan.  Test infrastructure only.
#include <string.h>
#include <vector>
#include "kzg_blob_lanes.h"
#include "lb_kzg_host.h"
#include "lb_kzg_transcript.h"

static fr rd_le(const uint8_t* b) { return fr_to_mont(kzg_fr_from_le32(b)); }
static fr rd_be(const uint8_t* b) {
  fr v;
  fr_from_be32(v, b);
  return v;
}
static void wr_words(uint8_t* b, const uint32_t* w) {
  for (int k = 0; k < 8; k++)
    for (int s = 0; s < 4; s++) b[4 * k + s] = (uint8_t)(w[k] >> (8 * s));
}

extern "C" {
void c_kzg_blob_challenge(const uint8_t* blob, const uint8_t* commitment48, uint8_t* z32be) {
  kzg_fr_to_be32(z32be, kzg_blob_challenge(blob, commitment48));
}
void c_kzg_blob_challenges(uint32_t n, const uint8_t* blobs, const uint8_t* commitments48, uint32_t threads, uint8_t* z32be) {
  std::vector<fr> z(n);
  kzg_blob_challenges(n, blobs, commitments48, z.data(), threads);
  for (uint32_t i = 0; i < n; i++) kzg_fr_to_be32(z32be + 32 * i, z[i]);
}
void c_kzg_batch_r(uint32_t n, const uint8_t* commitments48, const uint8_t* z32be, const uint8_t* y32be,
                   const uint8_t* proofs48, uint8_t* r32be) {
  std::vector<fr> z(n), y(n);
  for (uint32_t i = 0; i < n; i++) {
    z[i] = rd_be(z32be + 32 * i);
    y[i] = rd_be(y32be + 32 * i);
  }
  kzg_fr_to_be32(r32be, kzg_batch_r(n, commitments48, z.data(), y.data(), proofs48));
}
// n_polys polynomials of n coefficients, polynomial k at z[k]: q32 holds n_polys x n values (slot k
// at k * n, the last of each 0), y32 n_polys values
void c_fr_eval_quotient_many(uint32_t n_polys, uint32_t n, const uint8_t* coeffs, const uint8_t* z32, uint8_t* q32, uint8_t* y32) {
  std::vector<fr> a((size_t)n_polys * n), z(n_polys);
  for (size_t i = 0; i < a.size(); i++) a[i] = rd_le(coeffs + 32 * i);
  for (uint32_t k = 0; k < n_polys; k++) z[k] = rd_le(z32 + 32 * k);
  std::vector<uint32_t> q((size_t)8 * n_polys * n), y((size_t)8 * n_polys);
  eval_quotient_many_lanes(n_polys, n, a.data(), z.data(), q.data(), y.data());
  for (size_t i = 0; i < (size_t)n_polys * n; i++) wr_words(q32 + 32 * i, &q[8 * i]);
  for (uint32_t k = 0; k < n_polys; k++) wr_words(y32 + 32 * k, &y[8 * k]);
}
int32_t c_kzg_group_status(const int32_t* bstatus, const int32_t* tstatus, uint32_t n_blobs, uint32_t lo, uint32_t hi) {
  return kzg_group_status(bstatus, tstatus, n_blobs, lo, hi);
}
int32_t c_kzg_offsets_ok(uint32_t n, const uint32_t* off, uint32_t cap) { return kzg_offsets_ok(n, off, cap) ? 1 : 0; }
void c_kzg_fold_status(uint32_t n, const int32_t* first, const int32_t* second, int32_t* out_status, uint8_t* out0,
                       uint32_t stride0, uint8_t* out1, uint32_t stride1) {
  kzg_fold_status(n, first, second, out_status, out0, stride0, out1, stride1);
}
}
