// csrc/lb_ssz_walk.h and the root functions of csrc/lb_ssz_sets.h on the CPU: the code the GPU runs
// in lb_block_sets_from_ssz, on one thread (ssz_one_thread), driven by tests/test_ssz_sets_cpu.py.
//
//   ssz_walk_check <cases.bin>
//
// cases.bin: u32 count, then per case u32 fork, u32 flags (1 = skip proposer), u64 fork_epoch,
// u64 state_slot, 384 bytes of domains, u32 length, the bytes.  Every input is copied into a heap
// buffer of exactly its length and every scratch buffer has exactly the size the engine gives it,
// so a build with -fsanitize=address,undefined faults on any byte read outside the block and on any
// node written outside the scratch.  Prints, per case,
//   case <i> <status> <n_sets> <block root hex>
// and for an accepted block one line per set: <kind> <root> <signature> <ref0> <ref1> <ref2> <ref3>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lb_ssz_sets.h"

static void hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t zh[64 * 32];
  ssz_zero_hashes(zh, 64);
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t fork, flags, len;
    uint64_t fork_epoch, state_slot;
    uint8_t dom[384];
    if (fread(&fork, 4, 1, f) != 1 || fread(&flags, 4, 1, f) != 1 || fread(&fork_epoch, 8, 1, f) != 1 ||
        fread(&state_slot, 8, 1, f) != 1 || fread(dom, 384, 1, f) != 1 || fread(&len, 4, 1, f) != 1)
      return 2;
    uint8_t* ssz = (uint8_t*)malloc(len ? len : 1);  // exactly the block: the sanitizer sees every overrun
    if (len && fread(ssz, len, 1, f) != 1) return 2;
    if (!len) {  // a zero-length malloc may not be dereferenced at all
      free(ssz);
      ssz = (uint8_t*)malloc(0);
    }
    const bool skip = (flags & 1) != 0;
    ssz_blk k;
    ssz_index_block(ssz, 0, len, fork, k);
    const bool fail = !k.bad && k.sync_state == SSZ_SYNC_NOT_INFINITY;
    const uint32_t n = k.bad || fail ? 0 : ssz_n_sets(k, skip);
    uint32_t* N = (uint32_t*)malloc((size_t)LB_SSZ_N_NODES * 32);
    uint32_t* A = (uint32_t*)malloc((size_t)ssz_fold_cap(len) * 32);
    uint32_t* B = (uint32_t*)malloc((size_t)ssz_fold_cap(len) * 32);
    uint8_t root[32] = {0};
    if (!k.bad && !fail) {
      ssz_block_root(ssz_one_thread{}, ssz, k, N, A, B, zh);
      chunk_st(root, N + 8 * SN_BLOCK);
    }
    printf("case %u %d %u ", i, k.bad ? 1 : fail ? 5 : 0, n);
    hex(root, 32);
    printf("\n");
    for (uint32_t s = 0; s < n; s++) {
      uint32_t kind;
      uint8_t r32[32], sig[96];
      uint64_t ref[4];
      ssz_set_row(ssz, k, s, skip, dom, fork_epoch, state_slot, zh, N + 8 * SN_BLOCK, &kind, r32, sig, ref);
      printf("%u ", kind);
      hex(r32, 32);
      printf(" ");
      hex(sig, 96);
      printf(" %llu %llu %llu %llu\n", (unsigned long long)ref[0], (unsigned long long)ref[1],
             (unsigned long long)ref[2], (unsigned long long)ref[3]);
    }
    free(N);
    free(A);
    free(B);
    free(ssz);
  }
  fclose(f);
  printf("done %u\n", count);
  return 0;
}
