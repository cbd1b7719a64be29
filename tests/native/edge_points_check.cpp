// The point decoders, the compressors and the [r]P == O key validation of k_g1_decompress and
// k_table_fill over the records of tests/golden/edge_points.json, in a program of its own for a
// sanitizer build (tests/test_edge_points_cpu.py builds it with -fsanitize=address,undefined, writes
// the records as lines "<kind> <hex>" and compares what it prints with the fixture).  Each encoding
// is decoded from a heap block of exactly its size, so a read past 48 or 96 bytes is a report.
// Per record one line: <status> <inf> <in group: 0/1, - where not tested> <re-encoded hex or ->
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lb_serial.h"

static void put_hex(const uint8_t* b, int n) {
  for (int i = 0; i < n; i++) printf("%02x", b[i]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const uint32_t rr[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                          0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  char kind[16], hex[256];
  int n = 0;
  while (fscanf(f, "%15s %255s", kind, hex) == 2) {
    const size_t len = strlen(hex) / 2;
    uint8_t* b = (uint8_t*)malloc(len);
    for (size_t i = 0; i < len; i++) {
      unsigned v;
      sscanf(hex + 2 * i, "%2x", &v);
      b[i] = (uint8_t)v;
    }
    bool inf = false;
    int st;
    if (!strcmp(kind, "g2c96") && len == 96) {
      g2a a;
      st = g2_decompress96(b, a, inf);
      printf("%d %d - ", st, (int)inf);
      if (st == LB_OK) {
        uint8_t out[96];
        g2_compress96(out, a, inf);
        put_hex(out, 96);
      } else printf("-");
    } else if ((!strcmp(kind, "g1c48") && len == 48) || (!strcmp(kind, "g1u96") && len == 96)) {
      g1a a;
      st = len == 48 ? g1_decompress48(b, a, inf) : g1_deserialize96(b, a, inf);
      printf("%d %d ", st, (int)inf);
      if (st == LB_OK && !inf) printf("%d ", (int)jac_is_inf(jac_mul_u256(a, rr)));
      else printf("- ");
      if (st == LB_OK) {
        uint8_t out[96];
        if (len == 48) g1_compress48(out, a, inf);
        else g1_serialize96(out, a, inf);
        put_hex(out, (int)len);
      } else printf("-");
    } else {
      free(b);
      fclose(f);
      return 3;
    }
    printf("\n");
    free(b);
    n++;
  }
  fclose(f);
  printf("edge_points_check: records %d\n", n);
  return 0;
}
