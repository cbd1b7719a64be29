// Stand-alone check of the per-blob (Deneb) KZG calls' host and per-lane pieces for a sanitizer build
// (tests/test_kzg_blob_cpu.py builds it with -fsanitize=address,undefined and runs it): sha_stream
// against the FIPS 180 "abc" digest and against itself fed in odd pieces; kzg_blob_challenge and
// kzg_batch_r (n = 0, 1, 3) against the transcript assembled by hand; the threaded hashing of five
// blobs against one thread; the phases of k_fr_eval_quotient_many (kzg_blob_lanes.h) for three
// polynomials at three points against synthetic division, each in its own slot; and the status fold
// of k_kzg_check_groups over groups of 0, 1 and 3 blobs.  CPU only.
#include <stdio.h>
#include <vector>
#include "kzg_blob_lanes.h"
#include "lb_kzg_transcript.h"

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      failures++;                                                     \
      printf("kzg_blob_check: FAILED line %d: %s\n", __LINE__, #c);   \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static fr rnd_fr() {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = rng32();
  return fr_reduce256(w);
}
static fr digest_fr(const std::vector<uint8_t>& msg) {
  sha_stream s;
  s.update(msg.data(), msg.size());
  return kzg_digest_to_field(s);
}
static void put(std::vector<uint8_t>& v, const void* p, size_t n) {
  v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n);
}

int main() {
  const uint32_t n = 4096;
  // SHA-256
  {
    const uint8_t abc[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40, 0xde, 0x5d, 0xae, 0x22, 0x23,
                             0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17, 0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
    uint8_t d[32];
    sha_stream s;
    s.update((const uint8_t*)"abc", 3);
    s.finish(d);
    CHECK(memcmp(d, abc, 32) == 0);
    std::vector<uint8_t> msg(1000);
    for (uint8_t& b : msg) b = (uint8_t)rng32();
    uint8_t whole[32], pieces[32];
    sha_stream a, b;
    a.update(msg.data(), msg.size());
    a.finish(whole);
    for (size_t o = 0, k = 1; o < msg.size(); o += k, k = k % 97 + 7) b.update(msg.data() + o, std::min(k, msg.size() - o));
    b.finish(pieces);
    CHECK(memcmp(whole, pieces, 32) == 0);
  }
  // the transcripts
  std::vector<uint8_t> blobs(5 * LB_KZG_BLOB_BYTES), comms(5 * 48), proofs(5 * 48);
  for (uint8_t& b : blobs) b = (uint8_t)rng32();
  for (size_t i = 0; i < blobs.size(); i += 32) blobs[i] &= 0x3f;  // every element below r
  for (uint8_t& b : comms) b = (uint8_t)rng32();
  for (uint8_t& b : proofs) b = (uint8_t)rng32();
  std::vector<uint8_t> zero_blob(LB_KZG_BLOB_BYTES, 0);
  for (const uint8_t* blob : {(const uint8_t*)blobs.data(), (const uint8_t*)zero_blob.data()}) {
    std::vector<uint8_t> msg;
    uint8_t be[16] = {0};
    be[14] = 0x10;
    put(msg, "FSBLOBVERIFY_V1_", 16);
    put(msg, be, 16);
    put(msg, blob, LB_KZG_BLOB_BYTES);
    put(msg, comms.data(), 48);
    CHECK(fr_eq(kzg_blob_challenge(blob, comms.data()), digest_fr(msg)));
  }
  {
    std::vector<fr> z1(5), z3(5), z16(5);
    kzg_blob_challenges(5, blobs.data(), comms.data(), z1.data(), 1);
    kzg_blob_challenges(5, blobs.data(), comms.data(), z3.data(), 3);
    kzg_blob_challenges(5, blobs.data(), comms.data(), z16.data(), 16);
    for (uint32_t i = 0; i < 5; i++) {
      CHECK(fr_eq(z1[i], kzg_blob_challenge(blobs.data() + i * LB_KZG_BLOB_BYTES, comms.data() + 48 * i)));
      CHECK(fr_eq(z1[i], z3[i]));
      CHECK(fr_eq(z1[i], z16[i]));
    }
    std::vector<fr> y(5);
    for (fr& v : y) v = rnd_fr();
    y[0] = fr_zero();
    for (uint32_t cnt : {0u, 1u, 3u}) {
      std::vector<uint8_t> msg;
      uint8_t be[16] = {0};
      be[6] = 0x10;
      be[15] = (uint8_t)cnt;
      put(msg, "RCKZGBATCH___V1_", 16);
      put(msg, be, 16);
      for (uint32_t i = 0; i < cnt; i++) {
        uint8_t zy[64];
        kzg_fr_to_be32(zy, z1[i]);
        kzg_fr_to_be32(zy + 32, y[i]);
        put(msg, comms.data() + 48 * i, 48);
        put(msg, zy, 64);
        put(msg, proofs.data() + 48 * i, 48);
      }
      CHECK(msg.size() == 32 + 160 * (size_t)cnt);
      CHECK(fr_eq(kzg_batch_r(cnt, comms.data(), z1.data(), y.data(), proofs.data()), digest_fr(msg)));
    }
    // big-endian bytes round-trip
    uint8_t b32[32];
    kzg_fr_to_be32(b32, y[1]);
    fr back;
    CHECK(fr_from_be32(back, b32) && fr_eq(back, y[1]));
  }
  // three polynomials at three points, each in its own slot
  {
    const uint32_t rw[8] = LB_FR_ROOT4096_WORDS;
    const fr root = fr_to_mont(fr_from_words(rw));
    fr root5 = fr_one();
    for (int i = 0; i < 5; i++) root5 = fr_mul(root5, root);
    std::vector<fr> coef((size_t)3 * n, fr_zero());
    for (uint32_t i = 0; i < n; i++) coef[i] = rnd_fr();
    coef[(size_t)2 * n + n - 1] = rnd_fr();
    const fr zs[3] = {rnd_fr(), fr_zero(), root5};
    std::vector<uint32_t> q((size_t)3 * n * 8, 0xaaaaaaaau), y(3 * 8, 0xaaaaaaaau);
    eval_quotient_many_lanes(3, n, coef.data(), zs, q.data(), y.data());
    for (uint32_t k = 0; k < 3; k++) {
      fr acc = fr_zero();
      for (uint32_t j = n - 1; j > 0; j--) {
        acc = fr_add(fr_mul(acc, zs[k]), coef[(size_t)k * n + j]);
        uint32_t w[8];
        fr_to_le_words(w, acc);
        CHECK(memcmp(w, &q[((size_t)k * n + j - 1) * 8], 32) == 0);
      }
      acc = fr_add(fr_mul(acc, zs[k]), coef[(size_t)k * n]);
      uint32_t w[8];
      fr_to_le_words(w, acc);
      CHECK(memcmp(w, &y[8 * k], 32) == 0);
      for (int i = 0; i < 8; i++) CHECK(q[((size_t)k * n + n - 1) * 8 + i] == 0);
    }
  }
  // the status fold: groups of 0, 1 and 3 blobs
  {
    const uint32_t off[4] = {0, 0, 1, 4}, nb = 4, ng = 3;
    std::vector<int32_t> bst(nb, LB_OK), tst(3 * nb + ng, LB_OK);
    for (uint32_t k = 0; k < ng; k++) CHECK(kzg_group_status(bst.data(), tst.data(), nb, off[k], off[k + 1]) == LB_OK);
    for (uint32_t j = 0; j < nb; j++) {
      const uint32_t own = j == 0 ? 1 : 2;
      for (int kind = 0; kind < 3; kind++) {
        std::vector<int32_t> b = bst, t = tst;
        const int32_t code = kind == 0 ? LB_POINT_NOT_IN_GROUP : (kind == 1 ? LB_BAD_SCALAR : LB_BAD_ENCODING);
        if (kind == 0) t[j] = code;
        if (kind == 1) b[j] = code;
        if (kind == 2) t[nb + j] = t[2 * nb + j] = code;
        for (uint32_t k = 0; k < ng; k++)
          CHECK(kzg_group_status(b.data(), t.data(), nb, off[k], off[k + 1]) == (k == own ? code : LB_OK));
      }
    }
    std::vector<int32_t> b = bst, t = tst;
    b[3] = LB_BAD_SCALAR;
    t[nb + 2] = t[2 * nb + 2] = LB_POINT_NOT_IN_GROUP;
    CHECK(kzg_group_status(b.data(), t.data(), nb, 1, 4) == LB_POINT_NOT_IN_GROUP);
    t[2] = LB_BAD_ENCODING;
    CHECK(kzg_group_status(b.data(), t.data(), nb, 1, 4) == LB_BAD_ENCODING);
    b[1] = LB_BAD_SCALAR;
    CHECK(kzg_group_status(b.data(), t.data(), nb, 1, 4) == LB_BAD_SCALAR);
    t[1] = LB_POINT_NOT_IN_GROUP;
    CHECK(kzg_group_status(b.data(), t.data(), nb, 1, 4) == LB_POINT_NOT_IN_GROUP);
    CHECK(kzg_group_status(b.data(), t.data(), nb, 0, 1) == LB_OK);
  }
  printf("kzg_blob_check: failures %d\n", failures);
  return failures ? 1 : 0;
}
