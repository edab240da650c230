// Microbenchmark: issue cost of every VALU opcode class the four-chain kernel's sampling loop issues
// (hmc_rows.hip), at that kernel's occupancy: four waves per SIMD.  One block of 16 waves per CU (its
// dynamic LDS keeps a second block off the CU), eight independent chains per lane, the same loop
// around every opcode.  Cycles come from the counters the waves read themselves: s_memtime around the
// loop (clock64) and the 100 MHz s_memrealtime (wall_clock64) beside it, so the table states
//   * the cost per wave-instruction in s_memtime ticks: ticks of the wave / (instructions x 4 waves),
//   * the same relative to v_fma_f64 in the same run (no clock assumed),
//   * the rate the s_memtime counter ran at during the run, from the two counters' ratio.
// Stand-alone: hipcc --offload-arch=gfx950 -O3 -o instr_prices instr_prices.hip; run it once.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

constexpr int kThreads = 1024;          // 16 waves: four per SIMD
constexpr int kLdsBytes = 96 * 1024;    // more than half a CU's 160 KB: one block per CU
constexpr int kIters = 4096;            // loop trips
constexpr int kPerTrip = 16;            // instructions per trip (two per chain)

struct Ticks {
  long long core, wall;
};

#define OPERANDS                                                                                           \
  : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3), [d4] "+v"(d4), [d5] "+v"(d5), [d6] "+v"(d6), \
    [d7] "+v"(d7), [u0] "+v"(u0), [u1] "+v"(u1), [u2] "+v"(u2), [u3] "+v"(u3), [u4] "+v"(u4), [u5] "+v"(u5), \
    [u6] "+v"(u6), [u7] "+v"(u7), [w0] "+v"(w0), [w1] "+v"(w1), [w2] "+v"(w2), [w3] "+v"(w3)                 \
  : [sc] "s"(sc), [sd] "s"(sd), [lane] "v"(lane), [e0] "v"(e0), [e1] "v"(e1)                                 \
  : "vcc"

// ONE(i) is the instruction on chain i (0..7); a trip issues every chain twice.
#define PRICE_KERNEL(NAME, ONE)                                                                    \
  __global__ __launch_bounds__(kThreads) void NAME(Ticks* out, double* sink, unsigned sc, double sd) { \
    const unsigned lane = threadIdx.x & 63;                                                        \
    double d0 = 1.0 + lane, d1 = 2.0 + lane, d2 = 3.0 + lane, d3 = 4.0 + lane, d4 = 5.0 + lane,     \
           d5 = 6.0 + lane, d6 = 7.0 + lane, d7 = 8.0 + lane;                                      \
    unsigned u0 = lane, u1 = lane + 1, u2 = lane + 2, u3 = lane + 3, u4 = lane + 4, u5 = lane + 5,  \
             u6 = lane + 6, u7 = lane + 7;                                                         \
    unsigned long long w0 = lane, w1 = lane + 1, w2 = lane + 2, w3 = lane + 3;                     \
    const double e0 = 0.75 + 1e-3 * lane, e1 = 1.25;                                               \
    const long long w_a = wall_clock64(), c_a = clock64();                                         \
    for (int k = 0; k < kIters; ++k) {                                                             \
      asm volatile(ONE(0) ONE(1) ONE(2) ONE(3) ONE(4) ONE(5) ONE(6) ONE(7)                         \
                   ONE(0) ONE(1) ONE(2) ONE(3) ONE(4) ONE(5) ONE(6) ONE(7) OPERANDS);              \
    }                                                                                              \
    const long long c_b = clock64(), w_b = wall_clock64();                                         \
    if (lane == 0) out[(blockIdx.x * kThreads + threadIdx.x) / 64] = Ticks{c_b - c_a, w_b - w_a};   \
    const double s = d0 + d1 + d2 + d3 + d4 + d5 + d6 + d7 + (double)(u0 + u1 + u2 + u3 + u4 + u5 + u6 + u7) + \
                     (double)(w0 + w1 + w2 + w3);                                                  \
    if (s == 1234.5) sink[0] = s;                                                                  \
  }

#define D(i) "%[d" #i "]"
#define U(i) "%[u" #i "]"
// 64-bit integer destinations: four chains, each used by two of the eight slots
#define W(i) "%[w" #i "]"
#define W0 W(0)
#define W1 W(1)
#define W2 W(2)
#define W3 W(3)
#define W4 W(0)
#define W5 W(1)
#define W6 W(2)
#define W7 W(3)

#define I_FMA(i) "v_fma_f64 " D(i) ", " D(i) ", %[e0], %[e1]\n\t"
#define I_MUL(i) "v_mul_f64 " D(i) ", " D(i) ", %[e1]\n\t"
#define I_ADD(i) "v_add_f64 " D(i) ", " D(i) ", %[e1]\n\t"
#define I_MAX(i) "v_max_f64 " D(i) ", " D(i) ", %[e1]\n\t"
#define I_MAD64(i) "v_mad_u64_u32 " W##i ", vcc, " U(i) ", %[sc], 0\n\t"
#define I_BITOP3(i) "v_bitop3_b32 " U(i) ", " U(i) ", %[lane], %[sc] bitop3:0x96\n\t"
#define I_ALIGNBIT(i) "v_alignbit_b32 " U(i) ", %[sc], " U(i) ", 12\n\t"
#define I_AND(i) "v_and_b32_e32 " U(i) ", %[sc], " U(i) "\n\t"
#define I_BFE(i) "v_bfe_u32 " U(i) ", " U(i) ", 20, 11\n\t"
#define I_ANDOR(i) "v_and_or_b32 " U(i) ", " U(i) ", %[sc], %[lane]\n\t"
#define I_FREXPM(i) "v_frexp_mant_f64_e32 " D(i) ", " D(i) "\n\t"
#define I_FREXPE(i) "v_frexp_exp_i32_f64_e32 " U(i) ", " D(i) "\n\t"
#define I_CVT(i) "v_cvt_f64_i32_e32 " D(i) ", " U(i) "\n\t"
#define I_RSQ(i) "v_rsq_f64_e32 " D(i) ", " D(i) "\n\t"
#define I_MOV64(i) "v_mov_b64 " D(i) ", %[e0]\n\t"
#define I_MOV32(i) "v_mov_b32_e32 " U(i) ", %[lane]\n\t"
#define I_CNDMASK(i) "v_cndmask_b32_e32 " U(i) ", " U(i) ", %[lane], vcc\n\t"
#define I_DPPMOV(i) "v_mov_b32_dpp " U(i) ", " U(i) " row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
// always true (-1 < lane): EXEC stays all ones
#define I_CMPX(i) "v_cmpx_lt_i32_e32 vcc, -1, %[lane]\n\t"
#define I_ADDU32(i) "v_add_u32_e32 " U(i) ", %[lane], " U(i) "\n\t"

PRICE_KERNEL(k_fma_f64, I_FMA)
PRICE_KERNEL(k_mul_f64, I_MUL)
PRICE_KERNEL(k_add_f64, I_ADD)
PRICE_KERNEL(k_max_f64, I_MAX)
PRICE_KERNEL(k_mad_u64_u32, I_MAD64)
PRICE_KERNEL(k_bitop3_b32, I_BITOP3)
PRICE_KERNEL(k_alignbit_b32, I_ALIGNBIT)
PRICE_KERNEL(k_and_b32, I_AND)
PRICE_KERNEL(k_bfe_u32, I_BFE)
PRICE_KERNEL(k_and_or_b32, I_ANDOR)
PRICE_KERNEL(k_frexp_mant_f64, I_FREXPM)
PRICE_KERNEL(k_frexp_exp_i32_f64, I_FREXPE)
PRICE_KERNEL(k_cvt_f64_i32, I_CVT)
PRICE_KERNEL(k_rsq_f64, I_RSQ)
PRICE_KERNEL(k_mov_b64, I_MOV64)
PRICE_KERNEL(k_mov_b32, I_MOV32)
PRICE_KERNEL(k_cndmask_b32, I_CNDMASK)
PRICE_KERNEL(k_mov_b32_dpp, I_DPPMOV)
PRICE_KERNEL(k_cmpx_lt_i32, I_CMPX)
PRICE_KERNEL(k_add_u32, I_ADDU32)

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

typedef void (*Kernel)(Ticks*, double*, unsigned, double);

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int blocks = prop.multiProcessorCount;
  const int waves = blocks * kThreads / 64;
  Ticks* out;
  double* sink;
  CHECK(hipMalloc(&out, sizeof(Ticks) * waves));
  CHECK(hipMalloc(&sink, 8));
  std::vector<Ticks> h(waves);
  struct Row {
    const char* name;
    Kernel k;
  } rows[] = {{"v_fma_f64", k_fma_f64},           {"v_mul_f64", k_mul_f64},
              {"v_add_f64", k_add_f64},           {"v_max_f64", k_max_f64},
              {"v_mad_u64_u32", k_mad_u64_u32},   {"v_bitop3_b32", k_bitop3_b32},
              {"v_alignbit_b32", k_alignbit_b32}, {"v_and_b32", k_and_b32},
              {"v_bfe_u32", k_bfe_u32},           {"v_and_or_b32", k_and_or_b32},
              {"v_frexp_mant_f64", k_frexp_mant_f64}, {"v_frexp_exp_i32_f64", k_frexp_exp_i32_f64},
              {"v_cvt_f64_i32", k_cvt_f64_i32},   {"v_rsq_f64", k_rsq_f64},
              {"v_mov_b64", k_mov_b64},           {"v_mov_b32", k_mov_b32},
              {"v_cndmask_b32", k_cndmask_b32},   {"v_mov_b32_dpp", k_mov_b32_dpp},
              {"v_cmpx_lt_i32", k_cmpx_lt_i32},   {"v_add_u32", k_add_u32}};
  std::printf("# %s, %d CUs, one block of %d threads per CU (4 waves per SIMD), %d x %d instructions per wave\n",
              prop.gcnArchName, blocks, kThreads, kIters, kPerTrip);
  std::printf("# ticks: s_memtime ticks per wave-instruction = wave's ticks / (instructions x 4 waves per SIMD)\n");
  std::printf("%-22s %10s %10s %10s %12s\n", "opcode", "ticks", "max", "vs_fma", "tick_MHz");
  double fma = 0.0;
  for (const Row& r : rows) {
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(r.k), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    for (int rep = 0; rep < 2; ++rep) {   // the first run warms the clocks and the instruction cache
      hipLaunchKernelGGL(r.k, dim3(blocks), dim3(kThreads), kLdsBytes, 0, out, sink, 0x7FF00FFFu, 0.5);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(h.data(), out, sizeof(Ticks) * waves, hipMemcpyDeviceToHost));
    double core = 0.0, wall = 0.0, mx = 0.0;
    for (const Ticks& t : h) {
      core += (double)t.core;
      wall += (double)t.wall;
      if ((double)t.core > mx) mx = (double)t.core;
    }
    const double n = (double)kIters * kPerTrip * 4.0;
    const double ticks = core / waves / n;
    if (fma == 0.0) fma = ticks;
    std::printf("%-22s %10.3f %10.3f %10.3f %12.1f\n", r.name, ticks, mx / n, ticks / fma, core / wall * 100.0);
  }
  CHECK(hipFree(out));
  CHECK(hipFree(sink));
  return 0;
}
