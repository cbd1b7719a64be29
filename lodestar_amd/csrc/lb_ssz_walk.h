// Where things are in one SignedBeaconBlock's SSZ bytes (phase0, altair, bellatrix, capella): the
// layout walk behind lb_block_sets_from_ssz.  Range sync and gossip hand the node the block as SSZ
// bytes, and everything getBlockSignatureSets hashes (state-transition/src/signatureSets/index.ts)
// sits at offsets those bytes give without the state.
//
// Device-free: plain integer code that compiles for host and device, tested on the CPU against an
// independent decoder and under the address sanitizer (tests/native/ssz_walk_check.cpp).  The
// bytes are untrusted.  Every offset read from them is checked before it is used: a container's
// first offset equals its fixed-part size, offsets do not decrease and do not pass their
// container's end, a list of fixed-size items has a length that is a multiple of the item size, a
// list of variable-size items gives its count by a first offset that is a multiple of 4, every
// count is within the type's limit, and a bitlist ends in a non-zero byte.  No byte outside
// [start, end) of the block is read.  Positions are absolute byte positions in the call's buffer
// (below 2^26: lb_block_sets_from_ssz takes at most 64 MiB), so sums of two of them fit 32 bits.
#pragma once
#include <stdint.h>

#include "lb_common.h"

enum { SSZ_PHASE0 = 0, SSZ_ALTAIR, SSZ_BELLATRIX, SSZ_CAPELLA };

// fixed sizes (types/src/{phase0,altair,bellatrix,capella}/sszTypes.ts, mainnet preset)
#define SSZ_SIGNED_BLOCK_FIXED 100u    // offset(message) + signature
#define SSZ_BLOCK_FIXED 84u            // slot, proposer_index, parent_root, state_root, offset(body)
#define SSZ_BODY_LISTS 200u            // randao_reveal 96 + eth1_data 72 + graffiti 32, then five offsets
#define SSZ_BODY_SYNC 220u             // sync_aggregate (64 + 96) from altair on
#define SSZ_PROPOSER_SLASHING 416u     // two SignedBeaconBlockHeader of 112 + 96
#define SSZ_SIGNED_HEADER 208u
#define SSZ_ATT_FIXED 228u             // offset + AttestationData 128 + signature 96 (Attestation, IndexedAttestation)
#define SSZ_DEPOSIT 1240u              // proof 33 x 32 + DepositData 184
#define SSZ_SIGNED_EXIT 112u
#define SSZ_SIGNED_BLS_CHANGE 172u     // BLSToExecutionChange 76 + signature 96
#define SSZ_WITHDRAWAL 44u
#define SSZ_PAYLOAD_EXTRA_OFF 436u     // offset(extra_data) within the payload
#define SSZ_PAYLOAD_LOGS_BLOOM 116u
#define SSZ_PAYLOAD_TX_OFF 504u        // offset(transactions); capella: offset(withdrawals) follows
#define SSZ_MAX_TX 1048576u            // MAX_TRANSACTIONS_PER_PAYLOAD
#define SSZ_MAX_TX_BYTES 1073741824u   // MAX_BYTES_PER_TRANSACTION
#define SSZ_MAX_COMMITTEE 2048u        // MAX_VALIDATORS_PER_COMMITTEE

// sync aggregate of a block (processSyncCommittee.ts:58-111)
enum { SSZ_SYNC_ABSENT = 0, SSZ_SYNC_SET, SSZ_SYNC_EMPTY, SSZ_SYNC_NOT_INFINITY };

// One block's index: absolute positions, byte lengths and counts.  A list of fixed-size items is
// (position of item 0, count); a list of variable-size items is (position of its offset table,
// its end, count) and ssz_item gives an item's bytes.
struct ssz_blk {
  uint32_t bad;    // 0, or 1 = LB_BAD_ENCODING
  uint32_t fork;
  uint32_t start, end;
  uint32_t msg, body;            // message [msg, end), body [body, end)
  uint32_t ps, n_ps;             // proposer slashings (416 B each)
  uint32_t as, as_end, n_as;     // attester slashings (variable)
  uint32_t at, at_end, n_at;     // attestations (variable)
  uint32_t dp, n_dp;             // deposits (1240 B each)
  uint32_t ex, n_ex;             // voluntary exits (112 B each)
  uint32_t sync, sync_state;     // sync aggregate: position, SSZ_SYNC_*
  uint32_t pl, pl_end, pl_fixed; // execution payload (bellatrix on; pl = 0 before)
  uint32_t xd, xd_len;           // extra_data
  uint32_t tx, tx_end, n_tx;     // transactions (variable)
  uint32_t max_tx_chunks;        // the longest transaction's 32-byte chunks
  uint32_t wd, n_wd;             // withdrawals (44 B each, capella)
  uint32_t bc, n_bc;             // BLS-to-execution changes (172 B each, capella)
};

LB_HD uint32_t ssz_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
LB_HD uint64_t ssz_u64(const uint8_t* p) { return (uint64_t)ssz_u32(p) | ((uint64_t)ssz_u32(p + 4) << 32); }

LB_HD uint32_t ssz_body_fixed(uint32_t fork) {
  return fork == SSZ_PHASE0 ? 220u : fork == SSZ_ALTAIR ? 380u : fork == SSZ_BELLATRIX ? 384u : 388u;
}

// A list of variable-size items in [lo, hi): its count from the first offset (0 for an empty list).
// Checks the first offset only (a multiple of 4, the table within the list, count <= limit); the
// other offsets are checked per item by ssz_item.  false = bad encoding.
LB_HD bool ssz_var_list(const uint8_t* ssz, uint32_t lo, uint32_t hi, uint32_t limit, uint32_t* n) {
  *n = 0;
  if (hi == lo) return true;
  if (hi - lo < 4) return false;
  const uint32_t first = ssz_u32(ssz + lo);
  if (first == 0 || (first & 3) || first > hi - lo || first / 4 > limit) return false;
  *n = first / 4;
  return true;
}

// Item i of a checked variable-size list (i < count): its bytes [*a, *b).  Checks offset i and its
// successor: not below the table's end, not decreasing, not past the list's end.
LB_HD bool ssz_item(const uint8_t* ssz, uint32_t lo, uint32_t hi, uint32_t n, uint32_t i, uint32_t* a, uint32_t* b) {
  const uint32_t len = hi - lo;
  const uint32_t oa = ssz_u32(ssz + lo + 4 * i);
  const uint32_t ob = i + 1 < n ? ssz_u32(ssz + lo + 4 * (i + 1)) : len;
  if (oa < 4 * n || oa > ob || ob > len) return false;
  *a = lo + oa;
  *b = lo + ob;
  return true;
}

// An Attestation in [a, b): offset 228, then a bitlist that is non-empty, ends in a non-zero byte and
// holds at most 2048 bits.
LB_HD bool ssz_attestation_ok(const uint8_t* ssz, uint32_t a, uint32_t b) {
  if (b - a < SSZ_ATT_FIXED + 1 || ssz_u32(ssz + a) != SSZ_ATT_FIXED) return false;
  const uint32_t nb = b - a - SSZ_ATT_FIXED;
  const uint32_t last = ssz[b - 1];
  if (last == 0 || nb > SSZ_MAX_COMMITTEE / 8 + 1) return false;
  uint32_t top = 0;
  while ((last >> (top + 1)) != 0) top++;
  return 8 * (nb - 1) + top <= SSZ_MAX_COMMITTEE;
}

// bit length of a checked bitlist of nb bytes ending at `end`
LB_HD uint32_t ssz_bitlist_len(const uint8_t* ssz, uint32_t end, uint32_t nb) {
  const uint32_t last = ssz[end - 1];
  uint32_t top = 0;
  while ((last >> (top + 1)) != 0) top++;
  return 8 * (nb - 1) + top;
}

// An IndexedAttestation in [a, b): offset 228, then at most 2048 uint64 indices.
LB_HD bool ssz_indexed_attestation_ok(const uint8_t* ssz, uint32_t a, uint32_t b) {
  if (b - a < SSZ_ATT_FIXED || ssz_u32(ssz + a) != SSZ_ATT_FIXED) return false;
  const uint32_t nb = b - a - SSZ_ATT_FIXED;
  return (nb & 7) == 0 && nb / 8 <= SSZ_MAX_COMMITTEE;
}

// An AttesterSlashing in [a, b): two offsets (8, then the second attestation's), two
// IndexedAttestations.  at[0..1] / at_end[0..1] = their bytes.
LB_HD bool ssz_attester_slashing(const uint8_t* ssz, uint32_t a, uint32_t b, uint32_t at[2], uint32_t at_end[2]) {
  if (b - a < 8 || ssz_u32(ssz + a) != 8) return false;
  const uint32_t o2 = ssz_u32(ssz + a + 4);
  if (o2 < 8 || o2 > b - a) return false;
  at[0] = a + 8;
  at_end[0] = a + o2;
  at[1] = a + o2;
  at_end[1] = b;
  return ssz_indexed_attestation_ok(ssz, at[0], at_end[0]) && ssz_indexed_attestation_ok(ssz, at[1], at_end[1]);
}

// Attester slashing s of a checked block, attestation j: its bytes.  (The index pass checked them.)
LB_HD void ssz_slashing_attestation(const uint8_t* ssz, const ssz_blk& k, uint32_t s, uint32_t j, uint32_t* a,
                                    uint32_t* b) {
  uint32_t ia, ib, at[2], at_end[2];
  ssz_item(ssz, k.as, k.as_end, k.n_as, s, &ia, &ib);
  ssz_attester_slashing(ssz, ia, ib, at, at_end);
  *a = at[j];
  *b = at_end[j];
}

// A list of fixed-size items in [lo, hi).
LB_HD bool ssz_fixed_list(uint32_t lo, uint32_t hi, uint32_t item, uint32_t limit, uint32_t* n) {
  const uint32_t len = hi - lo;
  *n = len / item;
  return len % item == 0 && *n <= limit;
}

// The block's containers and lists, everything but the per-item checks of the attestations and the
// transactions (ssz_attestation_item_ok, ssz_tx_item_ok: one lane each on the device).  Sets k.bad.
LB_HD void ssz_index_top(const uint8_t* ssz, uint32_t start, uint32_t end, uint32_t fork, ssz_blk& k) {
  k = ssz_blk{};
  k.bad = 1;
  k.fork = fork;
  k.start = start;
  k.end = end;
  if (fork > SSZ_CAPELLA || end < start) return;
  const uint32_t fixed = ssz_body_fixed(fork);
  if (end - start < SSZ_SIGNED_BLOCK_FIXED + SSZ_BLOCK_FIXED + fixed) return;
  if (ssz_u32(ssz + start) != SSZ_SIGNED_BLOCK_FIXED) return;
  k.msg = start + SSZ_SIGNED_BLOCK_FIXED;
  if (ssz_u32(ssz + k.msg + 80) != SSZ_BLOCK_FIXED) return;
  k.body = k.msg + SSZ_BLOCK_FIXED;
  const uint32_t blen = end - k.body;
  // the body's variable fields in order: five operation lists, [payload], [BLS changes]
  uint32_t o[8];
  uint32_t nv = 5;
  for (uint32_t i = 0; i < 5; i++) o[i] = ssz_u32(ssz + k.body + SSZ_BODY_LISTS + 4 * i);
  if (fork >= SSZ_BELLATRIX) o[nv++] = ssz_u32(ssz + k.body + 380);
  if (fork >= SSZ_CAPELLA) o[nv++] = ssz_u32(ssz + k.body + 384);
  o[nv] = blen;
  if (o[0] != fixed) return;
  for (uint32_t i = 0; i < nv; i++)
    if (o[i] > o[i + 1]) return;  // o[nv] = blen closes the chain: every o[i] <= blen
  uint32_t p[8];
  for (uint32_t i = 0; i <= nv; i++) p[i] = k.body + o[i];
  k.ps = p[0];
  if (!ssz_fixed_list(p[0], p[1], SSZ_PROPOSER_SLASHING, 16, &k.n_ps)) return;
  k.as = p[1];
  k.as_end = p[2];
  if (!ssz_var_list(ssz, p[1], p[2], 2, &k.n_as)) return;
  for (uint32_t s = 0; s < k.n_as; s++) {
    uint32_t a, b, at[2], at_end[2];
    if (!ssz_item(ssz, k.as, k.as_end, k.n_as, s, &a, &b) || !ssz_attester_slashing(ssz, a, b, at, at_end)) return;
  }
  k.at = p[2];
  k.at_end = p[3];
  if (!ssz_var_list(ssz, p[2], p[3], 128, &k.n_at)) return;
  k.dp = p[3];
  if (!ssz_fixed_list(p[3], p[4], SSZ_DEPOSIT, 16, &k.n_dp)) return;
  k.ex = p[4];
  if (!ssz_fixed_list(p[4], p[5], SSZ_SIGNED_EXIT, 16, &k.n_ex)) return;
  if (fork >= SSZ_ALTAIR) {
    k.sync = k.body + SSZ_BODY_SYNC;
    uint32_t any = 0;
    for (uint32_t i = 0; i < 64; i++) any |= ssz[k.sync + i];
    if (any) {
      k.sync_state = SSZ_SYNC_SET;
    } else {
      uint32_t rest = ssz[k.sync + 64] ^ 0xC0u;  // G2_POINT_AT_INFINITY: 0xC0, then zeros
      for (uint32_t i = 1; i < 96; i++) rest |= ssz[k.sync + 64 + i];
      k.sync_state = rest ? SSZ_SYNC_NOT_INFINITY : SSZ_SYNC_EMPTY;
    }
  }
  if (fork >= SSZ_BELLATRIX) {
    k.pl = p[5];
    k.pl_end = p[6];
    k.pl_fixed = fork >= SSZ_CAPELLA ? 512u : 508u;
    const uint32_t plen = k.pl_end - k.pl;
    if (plen < k.pl_fixed) return;
    const uint32_t ox = ssz_u32(ssz + k.pl + SSZ_PAYLOAD_EXTRA_OFF), ot = ssz_u32(ssz + k.pl + SSZ_PAYLOAD_TX_OFF);
    const uint32_t ow = fork >= SSZ_CAPELLA ? ssz_u32(ssz + k.pl + SSZ_PAYLOAD_TX_OFF + 4) : plen;
    if (ox != k.pl_fixed || ot < ox || ow < ot || ow > plen) return;
    k.xd = k.pl + ox;
    k.xd_len = ot - ox;
    if (k.xd_len > 32) return;
    k.tx = k.pl + ot;
    k.tx_end = k.pl + ow;
    if (!ssz_var_list(ssz, k.tx, k.tx_end, SSZ_MAX_TX, &k.n_tx)) return;
    k.wd = k.pl + ow;
    if (fork >= SSZ_CAPELLA && !ssz_fixed_list(k.wd, k.pl_end, SSZ_WITHDRAWAL, 16, &k.n_wd)) return;
  }
  if (fork >= SSZ_CAPELLA) {
    k.bc = p[6];
    if (!ssz_fixed_list(p[6], p[7], SSZ_SIGNED_BLS_CHANGE, 16, &k.n_bc)) return;
  }
  k.bad = 0;
}

// attestation i of a block whose top-level walk passed: its offsets and its bitlist
LB_HD bool ssz_attestation_item_ok(const uint8_t* ssz, const ssz_blk& k, uint32_t i) {
  uint32_t a, b;
  return ssz_item(ssz, k.at, k.at_end, k.n_at, i, &a, &b) && ssz_attestation_ok(ssz, a, b);
}

// transaction i likewise; *chunks = its 32-byte chunks
LB_HD bool ssz_tx_item_ok(const uint8_t* ssz, const ssz_blk& k, uint32_t i, uint32_t* chunks) {
  uint32_t a, b;
  if (!ssz_item(ssz, k.tx, k.tx_end, k.n_tx, i, &a, &b) || b - a > SSZ_MAX_TX_BYTES) return false;
  *chunks = (b - a + 31) / 32;
  return true;
}

// The whole index on one thread (the host; the device spreads the two item loops over lanes).
LB_HD void ssz_index_block(const uint8_t* ssz, uint32_t start, uint32_t end, uint32_t fork, ssz_blk& k) {
  ssz_index_top(ssz, start, end, fork, k);
  if (k.bad) return;
  for (uint32_t i = 0; i < k.n_at; i++)
    if (!ssz_attestation_item_ok(ssz, k, i)) k.bad = 1;
  for (uint32_t i = 0; i < k.n_tx && !k.bad; i++) {
    uint32_t c;
    if (!ssz_tx_item_ok(ssz, k, i, &c)) k.bad = 1;
    else if (c > k.max_tx_chunks) k.max_tx_chunks = c;
  }
}

// Sets of an indexed block, in block_signature_sets' order: randao, proposer slashings (two each),
// attester slashings (two each), attestations, exits, proposer, sync aggregate, BLS changes.
LB_HD uint32_t ssz_n_sets(const ssz_blk& k, bool skip_proposer) {
  return 1 + 2 * k.n_ps + 2 * k.n_as + k.n_at + k.n_ex + (skip_proposer ? 0 : 1) +
         (k.sync_state == SSZ_SYNC_SET ? 1 : 0) + k.n_bc;
}
