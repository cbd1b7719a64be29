// Carrier for the operand-level checks of the many-lane engines (tools/, not product code): applies
// the device functions of lb_row.h (row engine), lb_wave.h (wave engine) and lb_group_exec.h
// (8-lane program engine) to records read from a file and writes their raw outputs.  It judges
// nothing: tests/test_lane_engines_gpu.py compares the outputs with exact integers and with the
// Python models (tests/lane_engine_vectors.py builds the records).
//
//   lanes_check IN OUT
//
// IN  (little-endian 32-bit words): [magic 0x4c414e45, n_sections], then per section
//       [op, n_records, in_words, out_words] followed by n_records * in_words words.
// OUT : per section, in the same order, n_records * out_words words (no headers).
// in_words / out_words must equal the operation's own (table below), or the program stops.
// One JSON line on stdout: records per operation.  Exit 0 only if every HIP call succeeded; after
// a HIP error nothing further is launched.
//
// Records (i32: signed limb words; fp: 12 words, a 2^384-Montgomery value; Fp12: 12 fp in slot
// order c{k/6}.c{(k%6)/2}.c{k%2}):
//   row operations, one 16-lane row per record, 64 records per workgroup of LBR_NT threads;
//   out = the 16 lanes of the result:
//     1 rp_mul      x[14] (replicated over the row), y[14] (lane k: y[k]; lanes 14, 15: 0)
//     2 r1_mul      v[14], w[14] (both distributed)          3 r1_sqr   v[14]
//     4 r_reduce    16 int64 sums (lo, hi words), one per lane (the limb sums and lanes 14, 15)
//     5 f_add  6 f_sub  7 f_neg  8 f_mul3  9 f_mul8  10 f_mul    a[14], b[14] (rfp values)
//    11 r_operand (red false: carries only)   12 r_operand (red true)
//                   n (1..8), 8 pair words (slot 0..7 | coef << 16), 8 slots x 14 limbs
//    17 r1_export   v[14] -> fp                 16 r1_import -> r1_export   fp -> 16 lanes, fp
//   13 r_canon      l[14] -> fp (one lane per record)
//   staged import / export, 16 records per workgroup (the staging slots):
//    14 r_export + r_fp_of_staged   l[14] (a slot) -> fp
//    15 r_stage_fp, r_import_staged, r_export, r_fp_of_staged   fp -> the slot's 16 words, fp
//   wave / group reductions, one lane per record, out = fp:
//    20 w_lin<LBW_MAXP> full 0   21 the same, full 1   22 w_lin<LBW_MAXL> full 0   23 full 1
//                   np, nn, then MAXN terms (value fp, coef): term i is pair i of the record, so
//                   the added terms are [0, np) and the subtracted ones [MAXN - nn, MAXN); the
//                   kernel puts term i of its lane into an LDS slot of its own
//    24 g_reduce full 0   25 full 1     pa[12], na[12] as uint64 (lo, hi words)
//   Fp12 level, one workgroup per record:
//    30 r_mul (a, b)  31 r_sqr  32 r_csqr  33 r_frob  34 r_frob2 -> Fp12   35 r_is_one  36 r_eq (a, b) -> 1 word
//    37 r_pdbl_fast chained: k, then X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1 -> 6 fp
//    40 w_mul (a, b)  41 w_sqr  42 w_frob  43 w_frob2  44 w_conj  45 w_inv -> Fp12   46 w_is_one -> 1 word
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define LB_KGROUP 99
#include "lb_kernels.h"

#define LC_MAGIC 0x4c414e45u
#define LC_MAX_CHAIN 128

// ---------------------------------------------------------------- row operations (one row per record)
__device__ __forceinline__ void lc_load14(const int32_t* p, int (&x)[14]) {
  LB_UNROLL for (int i = 0; i < 14; i++) x[i] = p[i];
}
template <int OP, int IW, int OW>
__global__ void __launch_bounds__(LBR_NT) k_lc_row(const int32_t* __restrict__ in, int32_t* __restrict__ out, int nrec) {
  const int k = r_limb(), rec = blockIdx.x * LBR_NROWS + r_row();
  __shared__ int32_t slots[(OP == 11 || OP == 12) ? LBR_NROWS * 8 * 16 + LBR_NROWS * 8 : 1];
  const bool act = rec < nrec;  // the same for the 16 lanes of a row
  const int32_t* r = in + (size_t)(act ? rec : 0) * IW;
  if constexpr (OP == 11 || OP == 12) {
    // this row's 8 slots at slot 8 row + j, its pair words after the slots
    const int row = r_row();
    lds_i32* S = r_lds(slots);
    for (int j = 0; j < 8; j++) S[16 * (8 * row + j) + k] = k < 14 ? r[9 + 14 * j + k] : 0;
    if (k < 8) {
      const int w = r[1 + k];
      S[LBR_NROWS * 8 * 16 + 8 * row + k] = (w & ~0xffff) | (8 * row + (w & 7));
    }
    __syncthreads();
    if (act) {
      const int n = min(max(r[0], 1), 8);
      out[(size_t)rec * OW + k] = r_operand(S, S + LBR_NROWS * 8 * 16 + 8 * row, n, k, OP == 12, r_plimb(k));
    }
    return;
  }
  if (!act) return;
  int32_t* o = out + (size_t)rec * OW;
  if constexpr (OP == 1) {
    int x[14];
    lc_load14(r, x);
    o[k] = rp_mul(x, k < 14 ? r[14 + k] : 0, k);
  } else if constexpr (OP == 2) {
    o[k] = r1_mul(k < 14 ? r[k] : 0, k < 14 ? r[14 + k] : 0, k);
  } else if constexpr (OP == 3) {
    o[k] = r1_sqr(k < 14 ? r[k] : 0, k);
  } else if constexpr (OP == 4) {
    const int64_t* a = reinterpret_cast<const int64_t*>(r);
    o[k] = r_reduce(a[k], k);
  } else if constexpr (OP >= 5 && OP <= 10) {
    const rfp a{k < 14 ? r[k] : 0}, b{k < 14 ? r[14 + k] : 0};
    const rfp v = OP == 5 ? f_add(a, b) : OP == 6 ? f_sub(a, b) : OP == 7 ? f_neg(a) : OP == 8 ? f_mul3(a) : OP == 9 ? f_mul8(a) : f_mul(a, b);
    o[k] = v.v;
  } else if constexpr (OP == 16) {
    fp a;
    LB_UNROLL for (int w = 0; w < 12; w++) a.v[w] = (uint32_t)r[w];
    const int v = r1_import(a, k);
    o[k] = v;
    const fp e = r1_export(v, k);
    if (k < 12) {
      uint32_t w = 0;
      LB_UNROLL for (int i = 0; i < 12; i++) w = k == i ? e.v[i] : w;
      o[16 + k] = (int32_t)w;
    }
  } else if constexpr (OP == 17) {
    const fp e = r1_export(k < 14 ? r[k] : 0, k);
    if (k < 12) {
      uint32_t w = 0;
      LB_UNROLL for (int i = 0; i < 12; i++) w = k == i ? e.v[i] : w;
      o[k] = (int32_t)w;
    }
  }
}

__global__ void __launch_bounds__(64) k_lc_canon(const int32_t* __restrict__ in, int32_t* __restrict__ out, int nrec) {
  const int rec = blockIdx.x * 64 + threadIdx.x;
  if (rec >= nrec) return;
  int32_t l[14];
  LB_UNROLL for (int i = 0; i < 14; i++) l[i] = in[(size_t)rec * 14 + i];
  const fp v = r_canon(l);
  LB_UNROLL for (int w = 0; w < 12; w++) out[(size_t)rec * 12 + w] = (int32_t)v.v[w];
}

// staged import / export: 16 records per workgroup
template <int OP, int IW, int OW>
__global__ void __launch_bounds__(LBR_NT) k_lc_staged(const int32_t* __restrict__ in, int32_t* __restrict__ out, int nrec) {
  LBR_SHARED(S);
  r_init(S);
  lds_i32* L = r_lds(S);
  const int t = r_tid(), rec = blockIdx.x * 16 + t;
  const int A = LBR_A(0);
  if constexpr (OP == 14) {
    if (t < 16 * 16) {
      const int e = t >> 4, k = t & 15, re = blockIdx.x * 16 + e;
      L[16 * (A + e) + k] = (re < nrec && k < 14) ? in[(size_t)re * IW + k] : 0;
    }
    r_sync();
  } else {
    if (t < 16) {
      fp a = fp_zero();
      if (rec < nrec) {
        LB_UNROLL for (int w = 0; w < 12; w++) a.v[w] = (uint32_t)in[(size_t)rec * IW + w];
      }
      r_stage_fp(S, t, a);
    }
    r_sync();
    r_import_staged(S, A, 16);
    if (t < 16 * 16) {
      const int e = t >> 4, k = t & 15, re = blockIdx.x * 16 + e;
      if (re < nrec) out[(size_t)re * OW + k] = L[16 * (A + e) + k];
    }
  }
  r_export(S, A, 16);
  if (t < 16 && rec < nrec) {
    const fp v = r_fp_of_staged(S, t);
    LB_UNROLL for (int w = 0; w < 12; w++) out[(size_t)rec * OW + (OP == 15 ? 16 : 0) + w] = (int32_t)v.v[w];
  }
}

// ---------------------------------------------------------------- wave / group reductions (one lane per record)
template <int MAXN, bool FULL>
__global__ void __launch_bounds__(64) k_lc_wlin(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int nrec) {
  constexpr int LANES = LBW_SPAD / MAXN, IW = 2 + 13 * MAXN;
  static_assert(LANES >= 1 && LANES <= 64, "lanes_check: w_lin lanes");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LBW_SLOT_WORDS];
  lds_fp* S = (lds_fp*)reinterpret_cast<fp*>(lds);
  const int lane = threadIdx.x, rec = blockIdx.x * LANES + lane;
  const bool act = lane < LANES && rec < nrec;
  int16_t pr[2 * MAXN];
  int np = 0, nn = 0;
  if (act) {
    const uint32_t* r = in + (size_t)rec * IW;
    np = (int)min(r[0], (uint32_t)MAXN);
    nn = (int)min(r[1], (uint32_t)(MAXN - np));
    for (int i = 0; i < MAXN; i++) {
      fp v;
      LB_UNROLL for (int w = 0; w < 12; w++) v.v[w] = r[2 + 13 * i + w];
      lds_st(S, lane * MAXN + i, v);
      pr[2 * i] = (int16_t)(lane * MAXN + i);
      pr[2 * i + 1] = (int16_t)(r[2 + 13 * i + 12] & 7);
    }
  }
  __syncthreads();
  if (act) {
    const fp v = w_lin<MAXN>(S, pr, np, nn, FULL);
    LB_UNROLL for (int w = 0; w < 12; w++) out[(size_t)rec * 12 + w] = v.v[w];
  }
}
template <bool FULL>
__global__ void __launch_bounds__(64) k_lc_greduce(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int nrec) {
  const int rec = blockIdx.x * 64 + threadIdx.x;
  if (rec >= nrec) return;
  const uint64_t* r = reinterpret_cast<const uint64_t*>(in) + (size_t)rec * 24;
  uint64_t pa[12], na[12];
  LB_UNROLL for (int j = 0; j < 12; j++) {
    pa[j] = r[j];
    na[j] = r[12 + j];
  }
  const fp v = g_reduce(pa, na, FULL);
  LB_UNROLL for (int w = 0; w < 12; w++) out[(size_t)rec * 12 + w] = v.v[w];
}

// ---------------------------------------------------------------- Fp12 level (one workgroup per record)
template <int OP, int IW, int OW>
__global__ void __launch_bounds__(LBR_NT) k_lc_row12(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LBR_SHARED(S);
  r_init(S);
  const uint32_t* r = in + (size_t)blockIdx.x * IW;
  uint32_t* o = out + (size_t)blockIdx.x * OW;
  const int A = LBR_A(0), B = LBR_A(1), D = LBR_A(2);
  if constexpr (OP == 37) {
    const int t = r_tid(), chain = (int)min(r[0], (uint32_t)LC_MAX_CHAIN);
    if (t < 6) {
      fp v;
      LB_UNROLL for (int w = 0; w < 12; w++) v.v[w] = r[1 + 12 * t + w];
      r_stage_fp(S, t, v);
    }
    r_sync();
    r_import_staged(S, A, 6);
    for (int i = 0; i < chain; i++) r_pdbl_fast(S, A, A);
    r_export(S, A, 6);
    if (t < 6) {
      const fp v = r_fp_of_staged(S, t);
      LB_UNROLL for (int w = 0; w < 12; w++) o[12 * t + w] = v.v[w];
    }
    return;
  }
  r_load_soa12(S, A, r, 1, 0);
  if constexpr (OP == 30 || OP == 36) r_load_soa12(S, B, r + 144, 1, 0);
  if constexpr (OP == 35 || OP == 36) {
    const bool v = OP == 35 ? r_is_one(S, A) : r_eq(S, A, B);
    if (r_tid() == 0) o[0] = v ? 1u : 0u;
  } else {
    if constexpr (OP == 30) r_mul(S, D, A, B);
    if constexpr (OP == 31) r_sqr(S, D, A);
    if constexpr (OP == 32) r_csqr(S, D, A);
    if constexpr (OP == 33) r_frob(S, D, A);
    if constexpr (OP == 34) r_frob2(S, D, A);
    r_store_soa12(S, D, o, 1, 0);
  }
}
template <int OP, int IW, int OW>
__global__ void __launch_bounds__(64) k_lc_wave12(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LBW_SHARED(S);
  w_init_consts(S);
  const uint32_t* r = in + (size_t)blockIdx.x * IW;
  uint32_t* o = out + (size_t)blockIdx.x * OW;
  const int A = LBW_A(0), B = LBW_A(1), D = LBW_A(2);
  w_load_soa12(S, A, r, 1, 0);
  if constexpr (OP == 40) w_load_soa12(S, B, r + 144, 1, 0);
  if constexpr (OP == 46) {
    const bool v = w_is_one(S, A);
    if (w_lane() == 0) o[0] = v ? 1u : 0u;
  } else {
    if constexpr (OP == 40) w_mul(S, D, A, B);
    if constexpr (OP == 41) w_sqr(S, D, A);
    if constexpr (OP == 42) w_frob(S, D, A);
    if constexpr (OP == 43) w_frob2(S, D, A);
    if constexpr (OP == 44) w_conj(S, D, A);
    if constexpr (OP == 45) w_inv(S, D, A, LBW_A(3), LBW_A(4), LBW_A(5));
    w_store_soa12(S, D, o, 1, 0);
  }
}

// ---------------------------------------------------------------- host
#define HIP_OK(call)                                                                         \
  do {                                                                                       \
    const hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                                  \
      fprintf(stderr, "lanes_check: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      exit(2);                                                                               \
    }                                                                                        \
  } while (0)

struct lc_op {
  int op, iw, ow;
  const char* name;
  void (*launch)(const void* in, void* out, int nrec);
};
template <int OP, int IW, int OW>
static void l_row(const void* in, void* out, int n) {
  hipLaunchKernelGGL((k_lc_row<OP, IW, OW>), dim3((n + LBR_NROWS - 1) / LBR_NROWS), dim3(LBR_NT), 0, 0, (const int32_t*)in, (int32_t*)out, n);
}
static void l_canon(const void* in, void* out, int n) {
  hipLaunchKernelGGL(k_lc_canon, dim3((n + 63) / 64), dim3(64), 0, 0, (const int32_t*)in, (int32_t*)out, n);
}
template <int OP, int IW, int OW>
static void l_staged(const void* in, void* out, int n) {
  hipLaunchKernelGGL((k_lc_staged<OP, IW, OW>), dim3((n + 15) / 16), dim3(LBR_NT), 0, 0, (const int32_t*)in, (int32_t*)out, n);
}
template <int MAXN, bool FULL>
static void l_wlin(const void* in, void* out, int n) {
  constexpr int LANES = LBW_SPAD / MAXN;
  hipLaunchKernelGGL((k_lc_wlin<MAXN, FULL>), dim3((n + LANES - 1) / LANES), dim3(64), 0, 0, (const uint32_t*)in, (uint32_t*)out, n);
}
template <bool FULL>
static void l_greduce(const void* in, void* out, int n) {
  hipLaunchKernelGGL((k_lc_greduce<FULL>), dim3((n + 63) / 64), dim3(64), 0, 0, (const uint32_t*)in, (uint32_t*)out, n);
}
template <int OP, int IW, int OW>
static void l_row12(const void* in, void* out, int n) {
  hipLaunchKernelGGL((k_lc_row12<OP, IW, OW>), dim3(n), dim3(LBR_NT), 0, 0, (const uint32_t*)in, (uint32_t*)out);
}
template <int OP, int IW, int OW>
static void l_wave12(const void* in, void* out, int n) {
  hipLaunchKernelGGL((k_lc_wave12<OP, IW, OW>), dim3(n), dim3(64), 0, 0, (const uint32_t*)in, (uint32_t*)out);
}
#define LC_WL(maxn) (2 + 13 * (maxn))
static const lc_op OPS[] = {
    {1, 28, 16, "rp_mul", l_row<1, 28, 16>},
    {2, 28, 16, "r1_mul", l_row<2, 28, 16>},
    {3, 14, 16, "r1_sqr", l_row<3, 14, 16>},
    {4, 32, 16, "r_reduce", l_row<4, 32, 16>},
    {5, 28, 16, "f_add", l_row<5, 28, 16>},
    {6, 28, 16, "f_sub", l_row<6, 28, 16>},
    {7, 28, 16, "f_neg", l_row<7, 28, 16>},
    {8, 28, 16, "f_mul3", l_row<8, 28, 16>},
    {9, 28, 16, "f_mul8", l_row<9, 28, 16>},
    {10, 28, 16, "f_mul", l_row<10, 28, 16>},
    {11, 121, 16, "r_operand_carry", l_row<11, 121, 16>},
    {12, 121, 16, "r_operand_red", l_row<12, 121, 16>},
    {13, 14, 12, "r_canon", l_canon},
    {14, 14, 12, "r_export", l_staged<14, 14, 12>},
    {15, 12, 28, "r_import_export", l_staged<15, 12, 28>},
    {16, 12, 28, "r1_import_export", l_row<16, 12, 28>},
    {17, 14, 12, "r1_export", l_row<17, 14, 12>},
    {20, LC_WL(LBW_MAXP), 12, "w_lin_maxp", l_wlin<LBW_MAXP, false>},
    {21, LC_WL(LBW_MAXP), 12, "w_lin_maxp_full", l_wlin<LBW_MAXP, true>},
    {22, LC_WL(LBW_MAXL), 12, "w_lin_maxl", l_wlin<LBW_MAXL, false>},
    {23, LC_WL(LBW_MAXL), 12, "w_lin_maxl_full", l_wlin<LBW_MAXL, true>},
    {24, 48, 12, "g_reduce", l_greduce<false>},
    {25, 48, 12, "g_reduce_full", l_greduce<true>},
    {30, 288, 144, "r_mul", l_row12<30, 288, 144>},
    {31, 144, 144, "r_sqr", l_row12<31, 144, 144>},
    {32, 144, 144, "r_csqr", l_row12<32, 144, 144>},
    {33, 144, 144, "r_frob", l_row12<33, 144, 144>},
    {34, 144, 144, "r_frob2", l_row12<34, 144, 144>},
    {35, 144, 1, "r_is_one", l_row12<35, 144, 1>},
    {36, 288, 1, "r_eq", l_row12<36, 288, 1>},
    {37, 73, 72, "r_pdbl_fast", l_row12<37, 73, 72>},
    {40, 288, 144, "w_mul", l_wave12<40, 288, 144>},
    {41, 144, 144, "w_sqr", l_wave12<41, 144, 144>},
    {42, 144, 144, "w_frob", l_wave12<42, 144, 144>},
    {43, 144, 144, "w_frob2", l_wave12<43, 144, 144>},
    {44, 144, 144, "w_conj", l_wave12<44, 144, 144>},
    {45, 144, 144, "w_inv", l_wave12<45, 144, 144>},
    {46, 144, 1, "w_is_one", l_wave12<46, 144, 1>},
};
#define LC_MAX_RECORDS 4096

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: lanes_check IN OUT\n");
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "lanes_check: cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<uint32_t> file;
  {
    uint32_t buf[4096];
    size_t n;
    while ((n = fread(buf, 4, 4096, f)) > 0) file.insert(file.end(), buf, buf + n);
    fclose(f);
  }
  if (file.size() < 2 || file[0] != LC_MAGIC) {
    fprintf(stderr, "lanes_check: bad header\n");
    return 1;
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) {
    fprintf(stderr, "lanes_check: cannot write %s\n", argv[2]);
    return 1;
  }
  constexpr int NOPS = sizeof(OPS) / sizeof(OPS[0]);
  long counts[NOPS] = {0};
  size_t pos = 2;
  for (uint32_t s = 0; s < file[1]; s++) {
    if (pos + 4 > file.size()) {
      fprintf(stderr, "lanes_check: truncated section header\n");
      return 1;
    }
    const uint32_t op = file[pos], nrec = file[pos + 1], iw = file[pos + 2], ow = file[pos + 3];
    pos += 4;
    int idx = -1;
    for (int i = 0; i < NOPS; i++)
      if ((uint32_t)OPS[i].op == op) idx = i;
    if (idx < 0 || (uint32_t)OPS[idx].iw != iw || (uint32_t)OPS[idx].ow != ow || nrec > LC_MAX_RECORDS ||
        (size_t)nrec * iw > file.size() - pos) {
      fprintf(stderr, "lanes_check: bad section %u (op %u, %u records, %u / %u words)\n", s, op, nrec, iw, ow);
      return 1;
    }
    if (nrec) {
      const size_t ib = (size_t)nrec * iw * 4, ob = (size_t)nrec * ow * 4;
      void *din, *dout;
      HIP_OK(hipMalloc(&din, ib));
      HIP_OK(hipMalloc(&dout, ob));
      HIP_OK(hipMemcpy(din, file.data() + pos, ib, hipMemcpyHostToDevice));
      HIP_OK(hipMemset(dout, 0, ob));
      OPS[idx].launch(din, dout, (int)nrec);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      std::vector<uint32_t> res((size_t)nrec * ow);
      HIP_OK(hipMemcpy(res.data(), dout, ob, hipMemcpyDeviceToHost));
      HIP_OK(hipFree(din));
      HIP_OK(hipFree(dout));
      if (fwrite(res.data(), 4, res.size(), fo) != res.size()) {
        fprintf(stderr, "lanes_check: short write\n");
        return 1;
      }
    }
    counts[idx] += nrec;
    pos += (size_t)nrec * iw;
  }
  if (fclose(fo) != 0) return 1;
  printf("{");
  bool first = true;
  for (int i = 0; i < NOPS; i++)
    if (counts[i]) {
      printf("%s\"%s\": %ld", first ? "" : ", ", OPS[i].name, counts[i]);
      first = false;
    }
  printf("}\n");
  return 0;
}
