// A block's signature sets from its SSZ bytes (lb_block_sets_from_ssz): every set's signing root,
// signature and key reference, computed where lb_ssz_walk.h found them, and hash_tree_root of the
// BeaconBlock for the proposer set folded by a whole workgroup rather than one lane.
//
// Three kernels, in a sequence that depends on nothing read back:
//   k_ssz_index       one workgroup per block: the top-level walk on one lane, then one lane per
//                     attestation and per transaction offset; writes the block's ssz_blk, status
//                     and set count.
//   k_ssz_block_root  one workgroup per block: hash_tree_root(BeaconBlock).  Item roots one lane
//                     each (attestations, slashings, deposits' data, exits, withdrawals, BLS changes),
//                     the byte ranges chunk-parallel: the transactions' packed leaves over all lanes
//                     at once and folded level by level (ssz_tx_roots), attesting indices, logs_bloom,
//                     the deposit proofs' leaf level and every list of item roots likewise
//                     (ssz_wg_fold).  Levels above the real chunks hash with the zero-subtree roots.
//   k_ssz_sets        one lane per set: the fixed-layout object root and H(object_root || domain).
//
// What bounds them: SHA-256 on a lane is a serial chain of ~6 000 integer instructions per tree node
// and a block's tree has a critical path of a few dozen nodes (log2 of the longest transaction, the
// 25 + 20 zero-subtree levels of a transaction and of the list, the payload, body and block
// containers), so the call is bound by that latency chain and by launch + copy overhead, not by
// VALU throughput or memory bandwidth: 32 blocks of 100 KB are 100 000 nodes, 0.6 G instructions,
// spread over 32 workgroups.  The input is read once from L2/HBM (bytes, not words: SSZ positions
// have no alignment), the scratch nodes are word-aligned.
//
// Everything but the kernels is LB_HD and runs on the CPU with the one-thread context
// (tests/native/ssz_walk_check.cpp).
#pragma once
#include "lb_ssz.h"
#include "lb_ssz_walk.h"

#define LB_SSZ_MAX_SETS 199u  // LB_BLOCK_MAX_SETS
#define LB_SSZ_WG 512         // lanes of the per-block workgroups

// ------------------------------------------------------------------ nodes
// A node is 8 big-endian-loaded words (chunk_ld's form).  Scratch nodes are stored as words.
LB_HD void nd_ld(uint32_t w[8], const uint32_t* p) {
  LB_UNROLL for (int i = 0; i < 8; i++) w[i] = p[i];
}
LB_HD void nd_st(uint32_t* p, const uint32_t w[8]) {
  LB_UNROLL for (int i = 0; i < 8; i++) p[i] = w[i];
}
LB_HD void nd_zero(uint32_t w[8]) {
  LB_UNROLL for (int i = 0; i < 8; i++) w[i] = 0;
}
// chunk of a packed byte range: `avail` bytes from pos belong to it, the rest is zero padding
LB_HD void ssz_chunk(uint32_t w[8], const uint8_t* ssz, uint32_t pos, uint32_t avail) {
  if (avail >= 32) {
    chunk_ld(w, ssz + pos);
    return;
  }
  nd_zero(w);
  for (uint32_t j = 0; j < avail; j++) w[j >> 2] |= (uint32_t)ssz[pos + j] << (24 - 8 * (j & 3));
}
LB_HD uint32_t ssz_bswap(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}
// uint64 (and a length mix-in): little-endian in the chunk's first 8 bytes
LB_HD void ssz_u64_chunk(uint32_t w[8], uint64_t v) {
  nd_zero(w);
  w[0] = ssz_bswap((uint32_t)v);
  w[1] = ssz_bswap((uint32_t)(v >> 32));
}
LB_HD void ssz_mix(uint32_t root[8], uint64_t len) {
  uint32_t lw[8];
  ssz_u64_chunk(lw, len);
  sha256_node(root, root, lw);
}
LB_HD void ssz_hash_zero(uint32_t root[8], const uint8_t* zh, uint32_t d) {
  uint32_t z[8];
  chunk_ld(z, zh + 32 * d);
  sha256_node(root, root, z);
}

// ------------------------------------------------------------------ fixed-layout object roots
// five leaves (AttestationData, BeaconBlockHeader, BeaconBlock): depth 3
LB_HD void ssz_root5(uint32_t o[8], const uint32_t l0[8], const uint32_t l1[8], const uint32_t l2[8],
                     const uint32_t l3[8], const uint32_t l4[8], const uint8_t* zh) {
  uint32_t a[8], b[8];
  sha256_node(a, l0, l1);
  sha256_node(b, l2, l3);
  sha256_node(a, a, b);
  chunk_ld(b, zh);
  sha256_node(b, l4, b);
  ssz_hash_zero(b, zh, 1);
  sha256_node(o, a, b);
}
LB_HD void ssz_root_sig96(uint32_t o[8], const uint8_t* ssz, uint32_t pos) {
  uint32_t a[8], b[8], z[8];
  chunk_ld(a, ssz + pos);
  chunk_ld(b, ssz + pos + 32);
  sha256_node(a, a, b);
  chunk_ld(b, ssz + pos + 64);
  nd_zero(z);
  sha256_node(b, b, z);
  sha256_node(o, a, b);
}
LB_HD void ssz_root_pubkey48(uint32_t o[8], const uint8_t* ssz, uint32_t pos) {
  uint32_t a[8], b[8];
  chunk_ld(a, ssz + pos);
  ssz_chunk(b, ssz, pos + 32, 16);
  sha256_node(o, a, b);
}
LB_HD void ssz_root_checkpoint(uint32_t o[8], const uint8_t* ssz, uint32_t pos) {
  uint32_t a[8], b[8];
  ssz_u64_chunk(a, ssz_u64(ssz + pos));
  chunk_ld(b, ssz + pos + 8);
  sha256_node(o, a, b);
}
// AttestationData, 128 B: slot, index, beacon_block_root, source, target
LB_HD void ssz_root_attestation_data(uint32_t o[8], const uint8_t* ssz, uint32_t pos, const uint8_t* zh) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8];
  ssz_u64_chunk(l0, ssz_u64(ssz + pos));
  ssz_u64_chunk(l1, ssz_u64(ssz + pos + 8));
  chunk_ld(l2, ssz + pos + 16);
  ssz_root_checkpoint(l3, ssz, pos + 48);
  ssz_root_checkpoint(l4, ssz, pos + 88);
  ssz_root5(o, l0, l1, l2, l3, l4, zh);
}
// BeaconBlockHeader, 112 B: slot, proposer_index, parent_root, state_root, body_root
LB_HD void ssz_root_header(uint32_t o[8], const uint8_t* ssz, uint32_t pos, const uint8_t* zh) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8];
  ssz_u64_chunk(l0, ssz_u64(ssz + pos));
  ssz_u64_chunk(l1, ssz_u64(ssz + pos + 8));
  chunk_ld(l2, ssz + pos + 16);
  chunk_ld(l3, ssz + pos + 48);
  chunk_ld(l4, ssz + pos + 80);
  ssz_root5(o, l0, l1, l2, l3, l4, zh);
}
// VoluntaryExit, 16 B: epoch, validator_index
LB_HD void ssz_root_exit(uint32_t o[8], const uint8_t* ssz, uint32_t pos) {
  uint32_t a[8], b[8];
  ssz_u64_chunk(a, ssz_u64(ssz + pos));
  ssz_u64_chunk(b, ssz_u64(ssz + pos + 8));
  sha256_node(o, a, b);
}
// BLSToExecutionChange, 76 B: validator_index, from_bls_pubkey (48), to_execution_address (20)
LB_HD void ssz_root_bls_change(uint32_t o[8], const uint8_t* ssz, uint32_t pos) {
  uint32_t a[8], b[8], z[8];
  ssz_u64_chunk(a, ssz_u64(ssz + pos));
  ssz_root_pubkey48(b, ssz, pos + 8);
  sha256_node(a, a, b);
  ssz_chunk(b, ssz, pos + 56, 20);
  nd_zero(z);
  sha256_node(b, b, z);
  sha256_node(o, a, b);
}
// container {message root, signature root} of the Signed* types
LB_HD void ssz_root_signed(uint32_t o[8], const uint32_t msg[8], const uint8_t* ssz, uint32_t sig) {
  uint32_t s[8];
  ssz_root_sig96(s, ssz, sig);
  sha256_node(o, msg, s);
}

// ------------------------------------------------------------------ one set
// domains32 of one block: [previous = 0 / current = 1 fork version][proposer, attester, randao,
// voluntary_exit, sync_committee, bls_to_execution_change]
enum { SSZ_DOM_PROPOSER = 0, SSZ_DOM_ATTESTER, SSZ_DOM_RANDAO, SSZ_DOM_EXIT, SSZ_DOM_SYNC, SSZ_DOM_BLS };
enum { SSZ_SET_RANDAO = 0, SSZ_SET_PROPOSER_SLASHING, SSZ_SET_ATTESTER_SLASHING, SSZ_SET_ATTESTATION,
       SSZ_SET_VOLUNTARY_EXIT, SSZ_SET_PROPOSER, SSZ_SET_SYNC_AGGREGATE, SSZ_SET_BLS_TO_EXECUTION_CHANGE };

// Set s (s < ssz_n_sets) of an indexed block: its kind, signing root, signature and key reference.
// block_root = hash_tree_root(BeaconBlock) as a node (read for the proposer set only).
LB_HD void ssz_set_row(const uint8_t* ssz, const ssz_blk& k, uint32_t s, bool skip_proposer, const uint8_t* dom,
                       uint64_t fork_epoch, uint64_t state_slot, const uint8_t* zh, const uint32_t* block_root,
                       uint32_t* kind, uint8_t* root32, uint8_t* sig96, uint64_t ref[4]) {
  const uint64_t slot = ssz_u64(ssz + k.msg), proposer = ssz_u64(ssz + k.msg + 8);
  uint32_t obj[8], dt, sig, kd;
  uint64_t ep;
  ref[0] = ref[1] = ref[2] = ref[3] = 0;
  const uint32_t n_prop = skip_proposer ? 0u : 1u, n_sync = k.sync_state == SSZ_SYNC_SET ? 1u : 0u;
  if (s < 1) {
    kd = SSZ_SET_RANDAO;
    ep = slot / 32;
    ssz_u64_chunk(obj, ep);
    dt = SSZ_DOM_RANDAO;
    sig = k.body;
    ref[0] = proposer;
  } else if ((s -= 1) < 2 * k.n_ps) {
    const uint32_t item = k.ps + SSZ_PROPOSER_SLASHING * (s / 2), h = item + SSZ_SIGNED_HEADER * (s % 2);
    kd = SSZ_SET_PROPOSER_SLASHING;
    ssz_root_header(obj, ssz, h, zh);
    ep = ssz_u64(ssz + h) / 32;
    dt = SSZ_DOM_PROPOSER;
    sig = h + 112;
    ref[0] = ssz_u64(ssz + item + 8);  // both headers against header 1's proposer
  } else if ((s -= 2 * k.n_ps) < 2 * k.n_as) {
    uint32_t a, b;
    ssz_slashing_attestation(ssz, k, s / 2, s % 2, &a, &b);
    kd = SSZ_SET_ATTESTER_SLASHING;
    ssz_root_attestation_data(obj, ssz, a + 4, zh);
    ep = ssz_u64(ssz + a + 4 + 88);
    dt = SSZ_DOM_ATTESTER;
    sig = a + 132;
    ref[1] = (b - a - SSZ_ATT_FIXED) / 8;
    ref[2] = a + SSZ_ATT_FIXED;
    ref[3] = b - a - SSZ_ATT_FIXED;
  } else if ((s -= 2 * k.n_as) < k.n_at) {
    uint32_t a = 0, b = 0;
    ssz_item(ssz, k.at, k.at_end, k.n_at, s, &a, &b);
    kd = SSZ_SET_ATTESTATION;
    ssz_root_attestation_data(obj, ssz, a + 4, zh);
    ep = ssz_u64(ssz + a + 4 + 88);
    dt = SSZ_DOM_ATTESTER;
    sig = a + 132;
    ref[0] = ssz_u64(ssz + a + 4);
    ref[1] = ssz_u64(ssz + a + 12);
    ref[2] = a + SSZ_ATT_FIXED;
    ref[3] = b - a - SSZ_ATT_FIXED;
  } else if ((s -= k.n_at) < k.n_ex) {
    const uint32_t e = k.ex + SSZ_SIGNED_EXIT * s;
    kd = SSZ_SET_VOLUNTARY_EXIT;
    ssz_root_exit(obj, ssz, e);
    ep = ssz_u64(ssz + e);
    dt = SSZ_DOM_EXIT;
    sig = e + 16;
    ref[0] = ssz_u64(ssz + e + 8);
  } else if ((s -= k.n_ex) < n_prop) {
    kd = SSZ_SET_PROPOSER;
    nd_ld(obj, block_root);
    ep = slot / 32;
    dt = SSZ_DOM_PROPOSER;
    sig = k.start + 4;
    ref[0] = proposer;
  } else if ((s -= n_prop) < n_sync) {
    kd = SSZ_SET_SYNC_AGGREGATE;
    chunk_ld(obj, ssz + k.msg + 16);  // the parent root, signed at the previous slot
    ep = ((slot > 1 ? slot : 1) - 1) / 32;
    dt = SSZ_DOM_SYNC;
    sig = k.sync + 64;
    ref[2] = k.sync;
    ref[3] = 64;
  } else {
    const uint32_t c = k.bc + SSZ_SIGNED_BLS_CHANGE * (s - n_sync);
    kd = SSZ_SET_BLS_TO_EXECUTION_CHANGE;
    ssz_root_bls_change(obj, ssz, c);
    ep = state_slot / 32;
    dt = SSZ_DOM_BLS;
    sig = c + 76;
    ref[2] = c + 8;
    ref[3] = 48;
  }
  uint32_t d[8];
  chunk_ld(d, dom + 32 * ((ep < fork_epoch ? 0u : 6u) + dt));
  sha256_node(obj, obj, d);  // computeSigningRoot: SigningData{object_root, domain}
  *kind = kd;
  chunk_st(root32, obj);
  for (uint32_t i = 0; i < 96; i++) sig96[i] = ssz[sig + i];
}

// ------------------------------------------------------------------ hash_tree_root(BeaconBlock)
// The code below runs on `nt` cooperating threads (tid = 0 .. nt-1) that meet at cx.sync(): a
// workgroup on the device, one thread on the host.
struct ssz_one_thread {
  uint32_t tid = 0, nt = 1;
  void sync() const {}
};

// per-block node scratch N (LB_SSZ_N_NODES nodes), by node index
enum {
  SN_RANDAO = 0, SN_ETH1, SN_PS_LIST, SN_AS_LIST, SN_AT_LIST, SN_DP_LIST, SN_EX_LIST, SN_SYNC, SN_PAYLOAD,
  SN_BC_LIST, SN_BLOCK, SN_LOGS_BLOOM, SN_EXTRA, SN_TX_LIST, SN_WD_LIST,
  SN_LEAVES = 16,   // 16 leaves of a container folded by lane 0
  SN_PS = 32,       // 16 proposer slashings
  SN_AS = 48,       // 2 attester slashings
  SN_AS_IDX = 50,   // their 4 attesting-index lists
  SN_AT = 64,       // 128 attestations
  SN_DP = 192,      // 16 deposits
  SN_EX = 208,      // 16 signed exits
  SN_WD = 224,      // 16 withdrawals
  SN_BC = 240,      // 16 signed BLS changes
  SN_PROOF = 256,   // 16 x 17 level-1 nodes of the deposit proofs
  LB_SSZ_N_NODES = 528
};

// Nodes both ping-pong buffers of a block need: the transactions' slots (data / 64 + count + 1, at
// most len / 4 + 1 since 4 * count + data <= len) and the small lists.
LB_HD uint32_t ssz_fold_cap(uint32_t block_len) { return block_len / 4 + 1024; }

// Root of a packed byte range (bytes != nullptr: nbytes of it at pos) or of nn nodes, padded to
// 2^depth leaves, optionally mixed with a length: all threads fold a level at a time, A and B in
// turn (the source is neither).  out = one node.
template <class Ctx>
LB_HD void ssz_wg_fold(const Ctx& cx, const uint8_t* bytes, uint32_t pos, uint32_t nbytes, const uint32_t* nodes,
                       uint32_t nn, uint32_t depth, uint64_t mix, uint32_t* A, uint32_t* B, const uint8_t* zh,
                       uint32_t* out) {
  uint32_t len = bytes ? (nbytes + 31) / 32 : nn;
  const uint32_t* cur = nullptr;
  uint32_t* dst = A;
  uint32_t d = 0;
  for (; d < depth && len > 1; d++) {
    const uint32_t half = (len + 1) / 2;
    for (uint32_t i = cx.tid; i < half; i += cx.nt) {
      uint32_t l[8], r[8];
      if (cur) nd_ld(l, cur + 16 * i);
      else if (bytes) ssz_chunk(l, bytes, pos + 64 * i, nbytes - 64 * i);
      else nd_ld(l, nodes + 16 * i);
      if (2 * i + 1 >= len) chunk_ld(r, zh + 32 * d);
      else if (cur) nd_ld(r, cur + 16 * i + 8);
      else if (bytes) ssz_chunk(r, bytes, pos + 64 * i + 32, nbytes - 64 * i - 32);
      else nd_ld(r, nodes + 16 * i + 8);
      sha256_node(l, l, r);
      nd_st(dst + 8 * i, l);
    }
    cx.sync();
    cur = dst;
    dst = dst == A ? B : A;
    len = half;
  }
  if (cx.tid == 0) {
    uint32_t root[8];
    if (len == 0) {
      chunk_ld(root, zh + 32 * depth);
    } else {
      if (cur) nd_ld(root, cur);
      else if (bytes) ssz_chunk(root, bytes, pos, nbytes);
      else nd_ld(root, nodes);
      for (; d < depth; d++) ssz_hash_zero(root, zh, d);
    }
    if (mix != LB_SSZ_NO_MIX) ssz_mix(root, mix);
    nd_st(out, root);
  }
  cx.sync();
}

// nodes of a tree of n0 chunks at level l (level 0 = the chunks)
LB_HD uint32_t ssz_level_nodes(uint32_t n0, uint32_t l) { return n0 == 0 ? 0 : ((n0 - 1) >> l) + 1; }

// Transaction i of a checked list: its offset from the list's start
LB_HD uint32_t ssz_tx_off(const uint8_t* ssz, const ssz_blk& k, uint32_t i) {
  return i < k.n_tx ? ssz_u32(ssz + k.tx + 4 * i) : k.tx_end - k.tx;
}
// ... and the slot its nodes start at in the fold buffers: data bytes before it / 64, plus i.  A
// transaction of L bytes has at most ceil(L / 64) nodes from level 1 up, and
// floor((a + L) / 64) + 1 >= floor(a / 64) + ceil(L / 64): the regions do not overlap.
LB_HD uint32_t ssz_tx_slot(const uint8_t* ssz, const ssz_blk& k, uint32_t i) {
  return (ssz_tx_off(ssz, k, i) - 4 * k.n_tx) / 64 + i;
}

// List[Transaction, 2^20] -> out.  Every transaction is List[byte, 2^30]: 2^25 leaves, then its
// length.  Level 1 hashes the packed bytes of all transactions at once, one lane per slot (the lane
// finds its transaction by bisection over the offsets, which the index pass found ordered); the
// levels up to the longest transaction's height fold all of them together, A and B in turn; then
// one lane per transaction climbs the zero-subtree levels and mixes the length in, and the list of
// roots is folded as any other.
template <class Ctx>
LB_HD void ssz_tx_roots(const Ctx& cx, const uint8_t* ssz, const ssz_blk& k, uint32_t* A, uint32_t* B,
                        const uint8_t* zh, uint32_t* out) {
  const uint32_t n = k.n_tx;
  uint32_t* cur = A;
  uint32_t* oth = B;
  if (n) {
    const uint32_t nslots = (k.tx_end - k.tx - 4 * n) / 64 + n + 1;
    uint32_t top = 1;  // levels folded together: ceil(log2(longest)), at least 1
    while (top < 25 && (1u << top) < k.max_tx_chunks) top++;
    for (uint32_t l = 1; l <= top; l++) {
      uint32_t* dst = (l & 1) ? A : B;
      const uint32_t* src = (l & 1) ? B : A;
      for (uint32_t j = cx.tid; j < nslots; j += cx.nt) {
        uint32_t lo = 0, hi = n;  // the last transaction whose first slot is <= j
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) / 2;
          if (ssz_tx_slot(ssz, k, mid) <= j) lo = mid;
          else hi = mid;
        }
        const uint32_t o = ssz_tx_off(ssz, k, lo), nb = ssz_tx_off(ssz, k, lo + 1) - o;
        const uint32_t s0 = (o - 4 * n) / 64 + lo, q = j - s0, n0 = (nb + 31) / 32;
        if (q >= ssz_level_nodes(n0, l)) continue;
        uint32_t a[8], b[8];
        if (l == 1) {
          ssz_chunk(a, ssz, k.tx + o + 64 * q, nb - 64 * q);
          if (2 * q + 1 < n0) ssz_chunk(b, ssz, k.tx + o + 64 * q + 32, nb - 64 * q - 32);
          else chunk_ld(b, zh);
        } else {
          nd_ld(a, src + 8 * (s0 + 2 * q));
          if (2 * q + 1 < ssz_level_nodes(n0, l - 1)) nd_ld(b, src + 8 * (s0 + 2 * q + 1));
          else chunk_ld(b, zh + 32 * (l - 1));
        }
        sha256_node(a, a, b);
        nd_st(dst + 8 * (s0 + q), a);
      }
      cx.sync();
    }
    cur = (top & 1) ? A : B;
    oth = (top & 1) ? B : A;
    for (uint32_t i = cx.tid; i < n; i += cx.nt) {
      const uint32_t o = ssz_tx_off(ssz, k, i), nb = ssz_tx_off(ssz, k, i + 1) - o;
      uint32_t root[8];
      if (nb == 0) {
        chunk_ld(root, zh + 32 * 25);
      } else {
        nd_ld(root, cur + 8 * ((o - 4 * n) / 64 + i));
        for (uint32_t d = top; d < 25; d++) ssz_hash_zero(root, zh, d);
      }
      ssz_mix(root, nb);
      nd_st(oth + 8 * i, root);  // i <= its slot: no root lands on a node another lane still reads
    }
    cx.sync();
  }
  ssz_wg_fold(cx, nullptr, 0, 0, oth, n, 20, (uint64_t)n, cur, oth, zh, out);
}

// lane 0: the container whose n leaves are at N[SN_LEAVES ..] (n <= 16), folded in place
LB_HD void ssz_container(uint32_t* N, uint32_t n, uint32_t depth, const uint8_t* zh, uint32_t* out) {
  uint32_t* c = N + 8 * SN_LEAVES;
  for (uint32_t d = 0; d < depth; d++) {
    const uint32_t half = (n + 1) / 2;
    for (uint32_t i = 0; i < half; i++) {
      uint32_t l[8], r[8];
      nd_ld(l, c + 16 * i);
      if (2 * i + 1 < n) nd_ld(r, c + 16 * i + 8);
      else chunk_ld(r, zh + 32 * d);
      sha256_node(l, l, r);
      nd_st(c + 8 * i, l);
    }
    n = half;
  }
  uint32_t root[8];
  nd_ld(root, c);
  nd_st(out, root);
}
LB_HD void ssz_leaf_bytes(uint32_t* N, uint32_t i, const uint8_t* ssz, uint32_t pos, uint32_t avail) {
  uint32_t w[8];
  ssz_chunk(w, ssz, pos, avail);
  nd_st(N + 8 * (SN_LEAVES + i), w);
}
LB_HD void ssz_leaf_u64(uint32_t* N, uint32_t i, const uint8_t* ssz, uint32_t pos) {
  uint32_t w[8];
  ssz_u64_chunk(w, ssz_u64(ssz + pos));
  nd_st(N + 8 * (SN_LEAVES + i), w);
}
LB_HD void ssz_leaf_node(uint32_t* N, uint32_t i, uint32_t node) {
  uint32_t w[8];
  nd_ld(w, N + 8 * node);
  nd_st(N + 8 * (SN_LEAVES + i), w);
}

// one-lane item roots of the first pass, by task
enum { TK_AT = 0, TK_PS = 128, TK_PROOF = 144, TK_EX = 416, TK_WD = 432, TK_BC = 448, TK_RANDAO = 464, TK_ETH1,
       TK_SYNC, TK_EXTRA, TK_N };

LB_HD void ssz_item_task(const uint8_t* ssz, const ssz_blk& k, uint32_t t, uint32_t* N, const uint8_t* zh) {
  uint32_t a[8], b[8], c[8];
  if (t < TK_PS) {  // Attestation {aggregation_bits, data, signature}
    const uint32_t i = t - TK_AT;
    if (i >= k.n_at) return;
    uint32_t p = 0, e = 0;
    ssz_item(ssz, k.at, k.at_end, k.n_at, i, &p, &e);
    const uint32_t nb = e - p - SSZ_ATT_FIXED, bits = ssz_bitlist_len(ssz, e, nb), bytes = (bits + 7) / 8;
    // the bits without the length marker: 8 chunks at most, folded here (depth 3), then the length
    uint32_t lv[4][8];
    const uint32_t bp = p + SSZ_ATT_FIXED, marker = bits >> 3, mbit = bits & 7;
    for (uint32_t j = 0; j < 4; j++) {
      uint32_t l[8], r[8];
      for (uint32_t h = 0; h < 2; h++) {
        uint32_t* w = h ? r : l;
        const uint32_t c0 = 32 * (2 * j + h);
        nd_zero(w);
        for (uint32_t x = 0; x < 32 && c0 + x < bytes; x++) {
          uint32_t v = ssz[bp + c0 + x];
          if (c0 + x == marker) v &= (1u << mbit) - 1;
          w[x >> 2] |= v << (24 - 8 * (x & 3));
        }
      }
      sha256_node(lv[j], l, r);
    }
    sha256_node(a, lv[0], lv[1]);
    sha256_node(b, lv[2], lv[3]);
    sha256_node(a, a, b);
    ssz_mix(a, bits);
    ssz_root_attestation_data(b, ssz, p + 4, zh);
    sha256_node(a, a, b);
    ssz_root_sig96(b, ssz, p + 132);
    nd_zero(c);
    sha256_node(b, b, c);
    sha256_node(a, a, b);
    nd_st(N + 8 * (SN_AT + i), a);
  } else if (t < TK_PROOF) {  // ProposerSlashing {signed_header_1, signed_header_2}
    const uint32_t i = t - TK_PS;
    if (i >= k.n_ps) return;
    const uint32_t p = k.ps + SSZ_PROPOSER_SLASHING * i;
    ssz_root_header(a, ssz, p, zh);
    ssz_root_signed(a, a, ssz, p + 112);
    ssz_root_header(b, ssz, p + SSZ_SIGNED_HEADER, zh);
    ssz_root_signed(b, b, ssz, p + SSZ_SIGNED_HEADER + 112);
    sha256_node(a, a, b);
    nd_st(N + 8 * (SN_PS + i), a);
  } else if (t < TK_EX) {  // a deposit proof's level 1: 33 chunks -> 17 nodes
    const uint32_t i = (t - TK_PROOF) / 17, j = (t - TK_PROOF) % 17;
    if (i >= k.n_dp) return;
    const uint32_t p = k.dp + SSZ_DEPOSIT * i + 64 * j;
    chunk_ld(a, ssz + p);
    if (j < 16) chunk_ld(b, ssz + p + 32);
    else nd_zero(b);
    sha256_node(a, a, b);
    nd_st(N + 8 * (SN_PROOF + 17 * i + j), a);
  } else if (t < TK_WD) {  // SignedVoluntaryExit
    const uint32_t i = t - TK_EX;
    if (i >= k.n_ex) return;
    const uint32_t p = k.ex + SSZ_SIGNED_EXIT * i;
    ssz_root_exit(a, ssz, p);
    ssz_root_signed(a, a, ssz, p + 16);
    nd_st(N + 8 * (SN_EX + i), a);
  } else if (t < TK_BC) {  // Withdrawal {index, validator_index, address, amount}
    const uint32_t i = t - TK_WD;
    if (i >= k.n_wd) return;
    const uint32_t p = k.wd + SSZ_WITHDRAWAL * i;
    ssz_u64_chunk(a, ssz_u64(ssz + p));
    ssz_u64_chunk(b, ssz_u64(ssz + p + 8));
    sha256_node(a, a, b);
    ssz_chunk(b, ssz, p + 16, 20);
    ssz_u64_chunk(c, ssz_u64(ssz + p + 36));
    sha256_node(b, b, c);
    sha256_node(a, a, b);
    nd_st(N + 8 * (SN_WD + i), a);
  } else if (t < TK_RANDAO) {  // SignedBLSToExecutionChange
    const uint32_t i = t - TK_BC;
    if (i >= k.n_bc) return;
    const uint32_t p = k.bc + SSZ_SIGNED_BLS_CHANGE * i;
    ssz_root_bls_change(a, ssz, p);
    ssz_root_signed(a, a, ssz, p + 76);
    nd_st(N + 8 * (SN_BC + i), a);
  } else if (t == TK_RANDAO) {
    ssz_root_sig96(a, ssz, k.body);
    nd_st(N + 8 * SN_RANDAO, a);
  } else if (t == TK_ETH1) {  // Eth1Data {deposit_root, deposit_count, block_hash}
    chunk_ld(a, ssz + k.body + 96);
    ssz_u64_chunk(b, ssz_u64(ssz + k.body + 128));
    sha256_node(a, a, b);
    chunk_ld(b, ssz + k.body + 136);
    nd_zero(c);
    sha256_node(b, b, c);
    sha256_node(a, a, b);
    nd_st(N + 8 * SN_ETH1, a);
  } else if (t == TK_SYNC) {  // SyncAggregate {bits (512), signature}
    if (k.fork < SSZ_ALTAIR) return;
    chunk_ld(a, ssz + k.sync);
    chunk_ld(b, ssz + k.sync + 32);
    sha256_node(a, a, b);
    ssz_root_signed(a, a, ssz, k.sync + 64);
    nd_st(N + 8 * SN_SYNC, a);
  } else if (t == TK_EXTRA) {  // extra_data: List[byte, 32], one chunk
    if (k.fork < SSZ_BELLATRIX) return;
    ssz_chunk(a, ssz, k.xd, k.xd_len);
    ssz_mix(a, k.xd_len);
    nd_st(N + 8 * SN_EXTRA, a);
  }
}

// Deposit i {proof, data}: the proof's 17 level-1 nodes up to depth 6, DepositData {pubkey,
// withdrawal_credentials, amount, signature}
LB_HD void ssz_deposit_task(const uint8_t* ssz, const ssz_blk& k, uint32_t i, uint32_t* N, const uint8_t* zh) {
  uint32_t* c = N + 8 * (SN_PROOF + 17 * i);
  uint32_t n = 17;
  for (uint32_t d = 1; d < 6; d++) {
    const uint32_t half = (n + 1) / 2;
    for (uint32_t j = 0; j < half; j++) {
      uint32_t l[8], r[8];
      nd_ld(l, c + 16 * j);
      if (2 * j + 1 < n) nd_ld(r, c + 16 * j + 8);
      else chunk_ld(r, zh + 32 * d);
      sha256_node(l, l, r);
      nd_st(c + 8 * j, l);
    }
    n = half;
  }
  uint32_t proof[8], a[8], b[8], s[8];
  nd_ld(proof, c);
  const uint32_t p = k.dp + SSZ_DEPOSIT * i + 1056;
  ssz_root_pubkey48(a, ssz, p);
  chunk_ld(b, ssz + p + 48);
  sha256_node(a, a, b);
  ssz_u64_chunk(b, ssz_u64(ssz + p + 80));
  ssz_root_sig96(s, ssz, p + 88);
  sha256_node(b, b, s);
  sha256_node(a, a, b);
  sha256_node(a, proof, a);
  nd_st(N + 8 * (SN_DP + i), a);
}

// hash_tree_root(BeaconBlock) of an indexed block -> N[SN_BLOCK].  N: LB_SSZ_N_NODES nodes; A, B:
// ssz_fold_cap(block length) nodes each.
template <class Ctx>
LB_HD void ssz_block_root(const Ctx& cx, const uint8_t* ssz, const ssz_blk& k, uint32_t* N, uint32_t* A, uint32_t* B,
                          const uint8_t* zh) {
  for (uint32_t t = cx.tid; t < TK_N; t += cx.nt) ssz_item_task(ssz, k, t, N, zh);
  cx.sync();
  for (uint32_t i = cx.tid; i < k.n_dp; i += cx.nt) ssz_deposit_task(ssz, k, i, N, zh);
  // attester slashings: the attesting indices chunk-parallel, the rest on lane 0
  for (uint32_t s = 0; s < k.n_as; s++) {
    uint32_t a[2], b[2];
    for (uint32_t j = 0; j < 2; j++) {
      ssz_slashing_attestation(ssz, k, s, j, &a[j], &b[j]);
      const uint32_t nb = b[j] - a[j] - SSZ_ATT_FIXED;
      ssz_wg_fold(cx, ssz, a[j] + SSZ_ATT_FIXED, nb, nullptr, 0, 9, (uint64_t)(nb / 8), A, B, zh,
                  N + 8 * (SN_AS_IDX + 2 * s + j));
    }
    if (cx.tid == 0) {
      uint32_t ia[2][8], x[8], y[8];
      for (uint32_t j = 0; j < 2; j++) {  // IndexedAttestation {attesting_indices, data, signature}
        nd_ld(ia[j], N + 8 * (SN_AS_IDX + 2 * s + j));
        ssz_root_attestation_data(x, ssz, a[j] + 4, zh);
        sha256_node(ia[j], ia[j], x);
        ssz_root_sig96(x, ssz, a[j] + 132);
        nd_zero(y);
        sha256_node(x, x, y);
        sha256_node(ia[j], ia[j], x);
      }
      sha256_node(x, ia[0], ia[1]);
      nd_st(N + 8 * (SN_AS + s), x);
    }
  }
  cx.sync();
  ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_PS, k.n_ps, 4, (uint64_t)k.n_ps, A, B, zh, N + 8 * SN_PS_LIST);
  ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_AS, k.n_as, 1, (uint64_t)k.n_as, A, B, zh, N + 8 * SN_AS_LIST);
  ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_AT, k.n_at, 7, (uint64_t)k.n_at, A, B, zh, N + 8 * SN_AT_LIST);
  ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_DP, k.n_dp, 4, (uint64_t)k.n_dp, A, B, zh, N + 8 * SN_DP_LIST);
  ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_EX, k.n_ex, 4, (uint64_t)k.n_ex, A, B, zh, N + 8 * SN_EX_LIST);
  if (k.fork >= SSZ_BELLATRIX) {
    ssz_wg_fold(cx, ssz, k.pl + SSZ_PAYLOAD_LOGS_BLOOM, 256, nullptr, 0, 3, LB_SSZ_NO_MIX, A, B, zh,
                N + 8 * SN_LOGS_BLOOM);
    ssz_tx_roots(cx, ssz, k, A, B, zh, N + 8 * SN_TX_LIST);
  }
  if (k.fork >= SSZ_CAPELLA) {
    ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_WD, k.n_wd, 4, (uint64_t)k.n_wd, A, B, zh, N + 8 * SN_WD_LIST);
    ssz_wg_fold(cx, nullptr, 0, 0, N + 8 * SN_BC, k.n_bc, 4, (uint64_t)k.n_bc, A, B, zh, N + 8 * SN_BC_LIST);
  }
  if (cx.tid == 0) {
    uint32_t nf = 8;
    if (k.fork >= SSZ_BELLATRIX) {  // ExecutionPayload: 14 fields, 15 with capella's withdrawals
      const uint32_t p = k.pl;
      ssz_leaf_bytes(N, 0, ssz, p, 32);         // parent_hash
      ssz_leaf_bytes(N, 1, ssz, p + 32, 20);    // fee_recipient
      ssz_leaf_bytes(N, 2, ssz, p + 52, 32);    // state_root
      ssz_leaf_bytes(N, 3, ssz, p + 84, 32);    // receipts_root
      ssz_leaf_node(N, 4, SN_LOGS_BLOOM);
      ssz_leaf_bytes(N, 5, ssz, p + 372, 32);   // prev_randao
      ssz_leaf_u64(N, 6, ssz, p + 404);         // block_number
      ssz_leaf_u64(N, 7, ssz, p + 412);         // gas_limit
      ssz_leaf_u64(N, 8, ssz, p + 420);         // gas_used
      ssz_leaf_u64(N, 9, ssz, p + 428);         // timestamp
      ssz_leaf_node(N, 10, SN_EXTRA);
      ssz_leaf_bytes(N, 11, ssz, p + 440, 32);  // base_fee_per_gas (uint256)
      ssz_leaf_bytes(N, 12, ssz, p + 472, 32);  // block_hash
      ssz_leaf_node(N, 13, SN_TX_LIST);
      if (k.fork >= SSZ_CAPELLA) ssz_leaf_node(N, 14, SN_WD_LIST);
      ssz_container(N, k.fork >= SSZ_CAPELLA ? 15 : 14, 4, zh, N + 8 * SN_PAYLOAD);
    }
    ssz_leaf_node(N, 0, SN_RANDAO);
    ssz_leaf_node(N, 1, SN_ETH1);
    ssz_leaf_bytes(N, 2, ssz, k.body + 168, 32);  // graffiti
    ssz_leaf_node(N, 3, SN_PS_LIST);
    ssz_leaf_node(N, 4, SN_AS_LIST);
    ssz_leaf_node(N, 5, SN_AT_LIST);
    ssz_leaf_node(N, 6, SN_DP_LIST);
    ssz_leaf_node(N, 7, SN_EX_LIST);
    if (k.fork >= SSZ_ALTAIR) ssz_leaf_node(N, nf++, SN_SYNC);
    if (k.fork >= SSZ_BELLATRIX) ssz_leaf_node(N, nf++, SN_PAYLOAD);
    if (k.fork >= SSZ_CAPELLA) ssz_leaf_node(N, nf++, SN_BC_LIST);
    uint32_t body[8], l0[8], l1[8], l2[8], l3[8];
    ssz_container(N, nf, nf > 8 ? 4 : 3, zh, N + 8 * SN_LEAVES);
    nd_ld(body, N + 8 * SN_LEAVES);
    ssz_u64_chunk(l0, ssz_u64(ssz + k.msg));
    ssz_u64_chunk(l1, ssz_u64(ssz + k.msg + 8));
    chunk_ld(l2, ssz + k.msg + 16);
    chunk_ld(l3, ssz + k.msg + 48);
    ssz_root5(l0, l0, l1, l2, l3, body, zh);
    nd_st(N + 8 * SN_BLOCK, l0);
  }
  cx.sync();
}

// ------------------------------------------------------------------ kernels
// per-block arguments of the call, uploaded with the bytes
struct ssz_blk_arg {
  uint32_t start, end, fork, pad;
  uint64_t fork_epoch, state_slot;
  uint64_t fold_off;  // first node of this block's A in the fold scratch; B follows A
};

#if defined(__HIPCC__)
struct ssz_workgroup {
  uint32_t tid, nt;
  __host__ __device__ void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

#if LB_KG(2)
__global__ void __launch_bounds__(LB_SSZ_WG) k_ssz_index(uint32_t n_blocks, const ssz_blk_arg* __restrict__ args,
                                                         const uint8_t* __restrict__ ssz, uint32_t skip_proposer,
                                                         ssz_blk* __restrict__ blks, int32_t* __restrict__ status,
                                                         uint32_t* __restrict__ n_sets) {
  __shared__ ssz_blk k;
  __shared__ uint32_t bad, maxc;
  const uint32_t b = blockIdx.x;
  if (b >= n_blocks) return;
  if (threadIdx.x == 0) {
    ssz_index_top(ssz, args[b].start, args[b].end, args[b].fork, k);
    bad = k.bad;
    maxc = 0;
  }
  __syncthreads();
  if (!bad) {
    for (uint32_t i = threadIdx.x; i < k.n_at; i += blockDim.x)
      if (!ssz_attestation_item_ok(ssz, k, i)) atomicOr(&bad, 1u);
    for (uint32_t i = threadIdx.x; i < k.n_tx; i += blockDim.x) {
      uint32_t c = 0;
      if (!ssz_tx_item_ok(ssz, k, i, &c)) atomicOr(&bad, 1u);
      else atomicMax(&maxc, c);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    k.bad = bad;
    k.max_tx_chunks = maxc;
    blks[b] = k;
    const bool fail = !bad && k.sync_state == SSZ_SYNC_NOT_INFINITY;  // "Empty sync committee signature is not infinity"
    status[b] = bad ? 1 /* LB_BAD_ENCODING */ : fail ? 5 /* LB_VERIFY_FAIL */ : 0;
    n_sets[b] = bad || fail ? 0 : ssz_n_sets(k, skip_proposer != 0);
  }
}
#endif  // LB_KG

#if LB_KG(2)
__global__ void __launch_bounds__(LB_SSZ_WG) k_ssz_block_root(uint32_t n_blocks, const ssz_blk_arg* __restrict__ args,
                                                              const uint8_t* __restrict__ ssz,
                                                              const ssz_blk* __restrict__ blks,
                                                              uint32_t* __restrict__ nodes, uint32_t* __restrict__ fold,
                                                              const uint8_t* __restrict__ zh) {
  const uint32_t b = blockIdx.x;
  if (b >= n_blocks) return;
  __shared__ ssz_blk k;
  if (threadIdx.x == 0) k = blks[b];
  __syncthreads();
  if (k.bad || k.sync_state == SSZ_SYNC_NOT_INFINITY) return;
  const ssz_workgroup cx{threadIdx.x, blockDim.x};
  uint32_t* A = fold + 8 * args[b].fold_off;
  ssz_block_root(cx, ssz, k, nodes + (size_t)8 * LB_SSZ_N_NODES * b, A, A + (size_t)8 * ssz_fold_cap(k.end - k.start), zh);
}
#endif  // LB_KG

#if LB_KG(2)
__global__ void __launch_bounds__(LB_TPB) k_ssz_sets(uint32_t n_blocks, const ssz_blk_arg* __restrict__ args,
                                                     const uint8_t* __restrict__ ssz, const uint8_t* __restrict__ domains,
                                                     uint32_t skip_proposer, const ssz_blk* __restrict__ blks,
                                                     const uint32_t* __restrict__ n_sets,
                                                     const uint32_t* __restrict__ nodes, const uint8_t* __restrict__ zh,
                                                     uint32_t* __restrict__ kind, uint8_t* __restrict__ roots,
                                                     uint8_t* __restrict__ sigs, uint64_t* __restrict__ ref) {
  const uint32_t t = lb_tid();
  const uint32_t b = t / LB_SSZ_MAX_SETS, s = t % LB_SSZ_MAX_SETS;
  if (b >= n_blocks || s >= n_sets[b]) return;
  const ssz_blk k = blks[b];
  uint64_t r[4];
  ssz_set_row(ssz, k, s, skip_proposer != 0, domains + (size_t)384 * b, args[b].fork_epoch, args[b].state_slot, zh,
              nodes + (size_t)8 * (LB_SSZ_N_NODES * b + SN_BLOCK), kind + t, roots + (size_t)32 * t, sigs + (size_t)96 * t, r);
  for (int i = 0; i < 4; i++) ref[(size_t)4 * t + i] = r[i];
}
#endif  // LB_KG
#endif  // __HIPCC__
