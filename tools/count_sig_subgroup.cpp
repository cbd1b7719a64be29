// The Fp multiplications of the signatures' subgroup ladder alone (k_sig_subgroup: Scott's test on one
// decoded signature), counted on the CPU build of the device headers like tests/harness/lb_count.cpp
// counts the stages (g++ -DLB_COUNT_OPS).  tools/count_ops.py subtracts it from the decode stage's
// count: a batch on the per-batch test does not run the ladder per set.
#define LB_COUNT_OPS 1
#include <string.h>
unsigned long long lb_count_mul = 0;
#include "lb_serial.h"

extern "C" unsigned long long cnt_sig_subgroup(const uint8_t* sig96) {
  g2a a;
  bool inf;
  const int st = g2_decompress96(sig96, a, inf);
  lb_count_mul = 0;
  if (st == 0 && !inf) g2_aff_in_subgroup_i(a);
  return lb_count_mul;
}
