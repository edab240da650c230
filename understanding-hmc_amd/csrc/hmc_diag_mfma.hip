// hmc_diag_mfma.hip — the one-read lag sums of hmc_diag_lags.hip on the matrix cores (complete
// passes, 96 <= n <= 208: c3's n = 200).
//
// The lag products are GEMM-shaped once the series is laid out as Hankel slices:
// v_mfma_f64_16x16x4_f64 with A[t'][k] = y_k[b + T + t'] and B[k][s] = y_k[b - s] (k = four split
// chains of ONE dimension, the contraction index) adds y_k[i] y_k[i + L] to entry (t', s) of tile T,
// L = T + t' + s, anchor i = b - s.  Tiles T = -16, 0, 16, .. and anchor steps b = 0, 16, ..: a lag
// L = 16 q + r gets s <= r from tile 16 q and s > r from tile 16 q - 16, so over all b every product
// y_i y_{i+L} (0 <= i, i + L < n; rows outside [0, n) are zeros in LDS) is added exactly once, and a
// tile only runs the anchor steps that still meet lags < n (the triangle, at 16-row granularity).
// V_t = sum_{s>=t} sq_s + sum_{s<=n-1-t} sq_s - 2 C_t with sq_s = sum_j y_{j,s}^2 (no cancellation
// in the square terms), y = x - x_j[0] per series as in lag_wave.
// Workgroup = 4 waves = 4 dimensions x a range of split chains (two workgroups per CU, so one's
// staging runs beside the other's matrix work): the waves stage each group of four split chains
// into LDS together (lanes across the 4 dims: 32-B row segments; each row's other segments are read
// by the neighbouring dimension groups on the same XCD), then each wave runs its dimension's tiles,
// accumulating across the range in registers (tiles x 4 doubles per lane).  Split means and stds come
// from the same A slices (partial sums over rows t' mod 16, reduced in a fixed order: deterministic,
// within a few ulps of np.mean's sequential sum).
#include <algorithm>

#include "hmc_diag.hpp"

namespace hmc {

namespace {

constexpr int kMfmaNT = 16;                      // tiles T = -16 .. 16 (kMfmaNT - 2)
constexpr int kMfmaMaxN = 16 * (kMfmaNT - 3);    // 208 samples per split chain (NTM = 14)
constexpr int kMfmaDims = 4;                     // waves (dimensions) per workgroup
constexpr int kMfmaThreads = 64 * kMfmaDims;
constexpr int kMfmaSer = 4 * kMfmaDims;          // series staged per chain group
constexpr int kMfmaSlack = 320;                  // doubles past the last series (read-ahead)
constexpr int kSqStride = 272;                   // sq rows per lane group (2176 B: bank-spread)
constexpr int kMfmaPW = kMfmaNT * 256 + 256 + 4; // partial doubles per wave: tiles, sq rows, moments

struct MfmaArgs {
  Src s;
  int P;            // LDS doubles between dims' series (rows -16 .. n + 29; 8 mod 32)
  int PK;           // between chains' (4 P + 16: 16 mod 32)
  int NT;           // tiles used
  int G;            // dimension groups ceil(D / kMfmaDims)
  int R;            // split-chain ranges (a multiple of 8)
  int64_t per;      // split chains per range (a multiple of 4)
};

// The small instance (NTM = 8, c4's halves) runs at three waves per SIMD (168 VGPRs: the B column
// read a step ahead instead of up front; three workgroups' double buffers in 141 KB of LDS):
// 41.40 -> 41.07 ms per c4 half against two waves (same box, alternating runs); more waves hide
// little here, the pass is not latency-bound the way that would
// VT >= 0 (NTM = 8 with 97 <= n <= 111, NTM = 14 with 193 <= n <= 207: VT = NTM - 2 = n / 16 and
// NT = NTM): the tile bound and the tile count are compile-time,
// so the triangle is static (no per-MFMA branches, no merges of accumulator tuples).  E4 (1..3,
// with VT): n % 16 < 12, and each anchor step's last tile runs as E4 v_mfma_f64_4x4x4 on the row
// groups that meet rows below n (a quarter of a 16x16x4's cycles each) instead of a whole tile.
template <int NTM, int E4 = 0, int VT = -1>
__global__ __launch_bounds__(kMfmaThreads) __attribute__((amdgpu_waves_per_eu(NTM <= 8 ? 3 : 2, NTM <= 8 ? 3 : 2))) void k_conv_mfma(MfmaArgs a,
                                                                                             double* partial) {
  // capacity of this instance: NTM tiles, NTM - 1 anchor steps, n <= 16 (NTM - 1)
  constexpr int kNB = NTM - 1, kRows = NTM - 1;
  // the host takes this instance for 16 (NTM - 3) < n <= 16 (NTM - 1) (launch_conv_mfma): slices
  // q <= kQAll always hold a row below n, and staging rows 16 i + 15 < n for i < kQAll (NTM = 6, below
  // the matrix-core range's lower bound, keeps every test)
  constexpr int kQAll = NTM == 6 ? -1 : NTM - 3;
  // LDS: [4 chains][dims] series of the group at k PK + w P (bank-spread for both the staging writes
  // and the matrix waves' slice reads), x0[16], slack, sq rows [dims][4 chain lanes][272]
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // XCD-major: the G dimension groups of one chain range run on one XCD (blocks id, id + 8, ..
  // share an XCD), so a row's segments are fetched into that L2 once
  const int id = blockIdx.x;
  const int local = id >> 3;
  const int r = (local / a.G) * 8 + (id & 7), g = local % a.G;
  const Src& s = a.s;
  const int n = s.n, D = s.D, P = a.P, PK = a.PK;
  // PIPE (n <= 144, where two sample buffers fit beside the other workgroup's): the staged group
  // g + 1 is written to the other LDS buffer while group g's matrix work runs from registers, and
  // group g + 1's operands are read into registers right after the group's one barrier -- no LDS
  // wait in front of the MFMAs and one barrier per group instead of two (c4's halves: 45.6 -> see
  // DESIGN.md §3.5).  (Two staged groups per pair of barriers: 48.1 -> 50.5 ms; a second
  // staging register set two groups ahead: 48.1 -> 48.3 ms.  Neither is kept.)
  constexpr bool PIPE = NTM <= 10;
  constexpr int NBUF = PIPE ? 2 : 1;
  constexpr bool SQR_LDS = NTM > 10;               // the sq rows live in LDS (else in registers)
  const int SB = 4 * PK;
  double* const x0l = lds + NBUF * SB;
  double* const sqb = x0l + NBUF * kMfmaSer + kMfmaSlack;
  const int64_t m2 = n_series(s);
  const int64_t jlo = (int64_t)r * a.per;
  const int64_t jhi = jlo + a.per < m2 ? jlo + a.per : m2;
  // split chains of this range (< 2^31), the group loop in 32-bit offsets o from jlo: its bounds
  // are scalar compares (int64 compares of wave-uniform values run on the VALU)
  const int nrem = jhi > jlo ? (int)(jhi - jlo) : 0;
  for (int i = tid; i < NBUF * (SB + kMfmaSer) + kMfmaSlack + (SQR_LDS ? kMfmaSer * kSqStride : 0); i += kMfmaThreads)
    lds[i] = 0.0;
  // staging role: wave = chain sk of the group, lane = (dim sw, row phase rho); rows rho + 16 i
  // (sk wave-uniform in an SGPR: the chain's base offset is scalar arithmetic)
  const int sk = uni(wv), sw = lane & 3, rho = lane >> 2;
  const int sd = g * kMfmaDims + sw;
  // staged rows of the next chain group (loads in flight under a group of matrix work)
  double xsa[kRows];
  double x0a = 0.0;
  // buffer loads based at the group's first split chain (uniform): one 32-bit lane offset (host-
  // checked below kLagOOB) plus 16 i rows (in the vector offset: the range check covers it); the
  // buffer ends with the view's last sample, so lanes past the range or the dims (offset kLagOOB)
  // and rows past the last chain's end read zeros (y = 0 - 0)
  const int rowb = (int)(s.sample_stride * 8);
  const double* const vend = split_ptr(s, m2 - 1, n - 1) + D;
  auto stage_load = [&](int o, double (&xs)[kRows], double& x0s) {
    const int64_t jg = jlo + o, j = jg + sk;
    const double* b = uni(split_ptr(s, jg, 0));
    const int64_t span = (vend - b) * 8;
    const int nrec = span < kLagOOB ? (int)span : kLagOOB;
    const int lo = (sd < D && o + sk < nrem) ? (int)((split_ptr(s, j, 0) - b) + sd) * 8 + rho * rowb : kLagOOB + 64;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(b), 0, nrec, 0x00020000);
    x0s = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, lo - rho * rowb, 0, 0));
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      xs[i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, lo + 16 * i * rowb, 0, 0));
  };
  // x0l holds x0 - S_d of each staged series (0 for chains past the range: their rows are zeros,
  // so their moments add nothing)
  const double Ssd = sd < D ? s.x[s.base + sd] : 0.0;
  auto stage_store = [&](int nn, const double (&xs)[kRows], double x0s, int buf, bool valid) {
    double* dst = lds + buf * SB + sk * PK + sw * P + 16 + rho;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (i < kQAll || 16 * i + 15 < nn) dst[16 * i] = xs[i] - x0s;      // whole 16-row phase
      else if (16 * i < nn && rho + 16 * i < nn) dst[16 * i] = xs[i] - x0s;   // rows >= n stay zero
    }
    if (rho == 0) x0l[buf * kMfmaSer + sk * 4 + sw] = valid ? x0s - Ssd : 0.0;
  };
  // matrix role: wave wv = dimension d; lane = (chain k = lane >> 4, t' or s = lane & 15)
  const int d = g * kMfmaDims + sk;
  const int k = lane >> 4, c16 = lane & 15;
  typedef double v4d __attribute__((ext_vector_type(4)));
  v4d acc[NTM];
#pragma unroll
  for (int t = 0; t < NTM; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  double* const sqa = sqb + (wv * 4 + k) * kSqStride;   // sq rows of this wave's chain lane group k
  // the small instances keep the sq rows in registers instead (they have the room: no LDS
  // read-modify-write per group)
  constexpr bool SQR = NTM <= 10;
  double sqr[SQR ? NTM : 1];
#pragma unroll
  for (int q = 0; q < (SQR ? NTM : 1); ++q) sqr[q] = 0.0;
  double a_std = 0.0, a_m = 0.0, a_m2 = 0.0;
  const int NT = a.NT;
  const double dn = n;
  const double rn = 1.0 / dn, rn1 = 1.0 / (dn - 1.0);
  // split moments, four groups at a time: after the row scans a group's totals (chain k: lane
  // 16 k + 15) are parked by one DPP row_shl:4 per value (lanes 3, 7, 11 take the previous three
  // groups' totals; lanes 12-15 the new ones), and the std/mean arithmetic runs once per four
  // groups on lanes 3, 7, 11, 15 of each row (the other lanes' results are never read)
  double pk1 = 0.0, pk2 = 0.0, pkx = 0.0;
  int gi = 0;                                     // groups parked (wave-uniform)
  auto park = [](double b, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(b), 0x104, 0xF, 0x7, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(b), 0x104, 0xF, 0x7, false);
    return __hiloint2double(hi, lo);
  };
  auto flush = [&]() {
    const double mm2 = pk2 - pk1 * (pk1 * rn);
    a_std += sqrt(mm2 > 0.0 ? mm2 * rn1 : 0.0);
    const double e = pkx + pk1 * rn;
    a_m += e;
    a_m2 = __builtin_fma(e, e, a_m2);
  };
  // the matrix operands of a group: A slices q = 0 .. NTM (rows 16 (q - 1) + 15 + t') and the B
  // column of every anchor step (NTM = 10; else one step ahead, read inside matrix)
  constexpr bool BBALL = PIPE && NTM > 8;          // every step's B column up front
  double sl[NTM + 1], bb[BBALL ? kNB : 1];
  auto ops_ptr = [&](int buf) {
    int zo = buf * SB + k * PK + wv * P + 16;     // (an opaque integer offset keeps sr an LDS pointer)
    asm volatile("" : "+v"(zo));
    return (const double*)(lds + zo);
  };
  auto read_ops = [&](int buf) {
    const double* sr = ops_ptr(buf);
#pragma unroll
    for (int q = 0; q <= NTM; ++q) sl[q] = sr[16 * (q - 1) + 15 + c16];
#pragma unroll
    for (int bi = 0; bi < (BBALL ? kNB : 1); ++bi) bb[bi] = sr[16 * bi + 15 - c16];
  };
  auto matrix = [&](int nn, int buf) {
    if (d < D) {
      const double* sr = ops_ptr(buf);
      // Anchor steps b = 16 bi + 15 (anchors b - 15 .. b: step 0 starts at anchor 0).  Every
      // product of tile ti (T = 16 (ti - 1)) at step bi pairs an anchor with row b + T + t' >=
      // 16 (bi + ti) - 1, so the tile meets a row below n only while 16 (bi + ti) <= n:
      // ti <= tl(bi) = n / 16 - bi (round 6: the bound was (n - 1) / 16 + 1 - bi, one tile per step
      // of LDS-zero rows unless 16 | n: 7 of 35 MFMAs per group at n = 99, 13 of 104 at
      // n = 200).  Steps bi <= v = (n - 1) / 16.  Step-major: a step's tiles are
      // independent accumulators back to back (a tile's own chain of dependent MFMAs ran 20-40 %
      // slower).  Tile ti at step bi reads A slice q = bi + ti (rows 16 (q - 1) + 15 + t'): the
      // slices q = 0 .. NTM are read once, up front, into registers; B of the next step is read a
      // step ahead.  Reads past row n + 29 land in the next series or the LDS slack, feed no MFMA.
      const int vt = nn >> 4;                     // tiles ti <= vt - bi meet rows below n
      if constexpr (!PIPE) read_ops(buf);
      double bcur = bb[0];
      auto bstep = [&](auto bi_c) {
        constexpr int bi = decltype(bi_c)::value;
        const int tl = min(NT - 1, vt - bi);
        double bnx = 0.0;
        if constexpr (BBALL) bnx = bi + 1 < kNB ? bb[bi + 1 < kNB ? bi + 1 : 0] : 0.0;
        else bnx = bi + 1 < kNB ? sr[16 * (bi + 1) + 15 - c16] : 0.0;
        auto tile = [&](auto ti_c) {
          constexpr int ti = decltype(ti_c)::value;
          if constexpr (bi + ti <= NTM) {
            constexpr int tls = VT - bi;          // (VT >= 0: the static bound)
            if (VT >= 0 ? (E4 > 0 ? ti < tls : ti <= tls) : ti <= tl) {
              acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(sl[bi + ti], bcur, acc[ti], 0, 0, 0);
            }
            else if (VT >= 0 && E4 > 0 && ti == tls) {
              // the step's edge tile: rows 16 (bi + ti) - 1 + t' < n only for t' <= n % 16, i.e.
              // accumulator components g < e4 (rows 4 g .. 4 g + 3).  Each takes one
              // v_mfma_f64_4x4x4f64 (a quarter of the 16x16x4 cost): its four blocks share the A
              // rows (A lane (k, blk, i) = y_k[row 4 g + i]), B is the 16x16x4 operand as it is
              // (lane (k, s)), and its result lane (i, blk, j) is entry (4 g + i, 4 blk + j) --
              // the lane and component g where the 16x16x4 layout keeps that entry.
#pragma unroll
              for (int g = 0; g < (E4 > 0 ? E4 : 1); ++g) {
                if constexpr (E4 > 0) {
                  const double a4 = sr[16 * (bi + ti - 1) + 15 + 4 * g + (c16 & 3)];
                  acc[ti][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(a4, bcur, acc[ti][g], 0, 0, 0);
                }
              }
            }
          }
        };
        static_for<NTM>(tile);
        bcur = bnx;
      };
      static_for<kNB>(bstep);
      // split moments of chain k and the sq rows from the slices q = 0 .. kRows (rows
      // 16 (q - 1) + 15 + t': every row once; row -1 and rows >= n are zeros or masked), the 16 row
      // phases reduced in a fixed xor order
      double ps1, ps2;
      double sv[kRows + 1];
#pragma unroll
      for (int q = 0; q <= kRows; ++q) sv[q] = SQR ? 0.0 : sqa[16 * q + c16];
      const int qn = nn >> 4;                     // slices past q = n / 16 hold rows >= n only
#pragma unroll
      for (int q = 0; q <= kRows; ++q) {
        // (rows n .. n + 29 of slice qn are LDS zeros; later slices may read the next series).
        // Only the last slices of an instance can lie past qn (kQAll): one select there, instead of
        // a guarded update per slice that the compiler turned into six v_cndmask per slice
        double y = sl[q];
        if (q > kQAll) y = q <= qn ? y : 0.0;
        if (q == 0) {                             // (no add to a zero start)
          ps1 = y;
          ps2 = y * y;
        } else {
          ps1 += y;
          ps2 = __builtin_fma(y, y, ps2);
        }
        if constexpr (SQR) sqr[q] = __builtin_fma(y, y, sqr[q]);
        else if (q <= kQAll || q <= qn) sqa[16 * q + c16] = __builtin_fma(y, y, sv[q]);   // sq row 16 q + t' - 1
      }
      // the 16 row phases of chain k summed by a DPP row_shr scan: the total lands in the row's
      // lane 15 (other lanes keep partial sums, accumulate into moments that are never read)
      ps1 += dpp_u<0x111>(ps1);
      ps2 += dpp_u<0x111>(ps2);
      ps1 += dpp_u<0x112>(ps1);
      ps2 += dpp_u<0x112>(ps2);
      ps1 += dpp_u<0x114>(ps1);
      ps2 += dpp_u<0x114>(ps2);
      ps1 += dpp_u<0x118>(ps1);
      ps2 += dpp_u<0x118>(ps2);
      pk1 = park(pk1, ps1);
      pk2 = park(pk2, ps2);
      pkx = park(pkx, x0l[buf * kMfmaSer + k * 4 + wv]);
      if ((gi & 3) == 3) flush();
      ++gi;
    }
  };
  if (nrem > 0) stage_load(0, xsa, x0a);
  if constexpr (PIPE) {
    // group jg in buffer buf: its operands are in registers when the iteration starts; the group
    // jg + 4 is stored into buf ^ 1 (last read before the previous iteration's barrier) and read
    // back after this iteration's barrier; the loads of group jg + 8 are issued before the matrix
    // work and waited for before the barrier
    if (nrem > 0) {
      __syncthreads();                            // the zeroed LDS
      stage_store(n, xsa, x0a, 0, sk < nrem);
      if (4 < nrem) stage_load(4, xsa, x0a);
      __syncthreads();
      if (d < D) read_ops(0);
    }
    int buf = 0;
    for (int o = 0; o < nrem; o += 4) {
      int nn = n;                                 // opaque per group: bounds recomputed, not hoisted
      asm volatile("" : "+s"(nn));
      if (o + 4 < nrem) {
        stage_store(nn, xsa, x0a, buf ^ 1, o + 4 + sk < nrem);
        if (o + 8 < nrem) stage_load(o + 8, xsa, x0a);
      }
      matrix(nn, buf);
      // the loads just issued land before the barrier: the workgroups that read one row's 128-B
      // lines stay in step and share them in L2.  FETCH_SIZE at c4's halves: 2.5x the samples
      // without this wait (44.9 ms), 1.3x with it (43.2 ms); loads three groups ahead in two
      // register sets with a wait for the older set: 2.0x, 44.1 ms
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                            // group jg + 4 stored, group jg read
      buf ^= 1;
      if (o + 4 < nrem && d < D) read_ops(buf);
    }
  } else {
    for (int o = 0; o < nrem; o += 4) {
      int nn = n;                                 // opaque per group: bounds recomputed, not hoisted
      asm volatile("" : "+s"(nn));
      __syncthreads();                            // the previous group's slices are read
      stage_store(nn, xsa, x0a, 0, o + sk < nrem);
      __syncthreads();
      if (o + 4 < nrem) stage_load(o + 4, xsa, x0a);    // in flight under this group's matrix work
      matrix(nn, 0);
    }
  }
  if (d < D && (gi & 3) != 0) {                   // the last groups: zero-padded to four
    while ((gi & 3) != 0) {
      pk1 = park(pk1, 0.0);
      pk2 = park(pk2, 0.0);
      pkx = park(pkx, 0.0);
      ++gi;
    }
    flush();
  }
  // partial of this wave: tiles (entry t' * 16 + s), sq rows (summed over the 4 chain lanes; LDS
  // entry i holds row i - 1), moments
  double* out = partial + ((int64_t)id * kMfmaDims + wv) * kMfmaPW;
#pragma unroll
  for (int t = 0; t < NTM; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[t * 256 + q * 64 + lane] = acc[t][q];
  if constexpr (SQR) {                            // rows 16 q + t' - 1, summed over the 4 lane groups
#pragma unroll
    for (int q = 0; q <= kRows; ++q) {
      double v = sqr[q];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int row = 16 * q + c16 - 1;
      if (lane < 16 && row >= 0) out[kMfmaNT * 256 + row] = v;
    }
  } else {
    const double* sw4 = sqb + wv * 4 * kSqStride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 64 * i + lane;              // output row; LDS entry row + 1
      double v = 0.0;
      if (row < 255)
        v = ((sw4[row + 1] + sw4[kSqStride + row + 1]) + sw4[2 * kSqStride + row + 1]) + sw4[3 * kSqStride + row + 1];
      out[kMfmaNT * 256 + row] = v;
    }
  }
  // moments: lanes 3, 7, 11, 15 of each row (the parked slots)
  auto slots = [&](double v) {
    v = (c16 & 3) == 3 ? v : 0.0;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
  };
  a_std = slots(a_std);
  a_m = slots(a_m);
  a_m2 = slots(a_m2);
  if (lane == 63) {
    out[kMfmaNT * 256 + 256] = a_std;
    out[kMfmaNT * 256 + 257] = a_m;
    out[kMfmaNT * 256 + 258] = a_m2;
  }
}

// red[d][e] = sum over the chain ranges (in order) of the partial entry e of dimension d's wave
__global__ __launch_bounds__(256) void k_mfma_ranges(MfmaArgs a, const double* __restrict__ partial,
                                                     double* __restrict__ red) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.s.D * kMfmaPW) return;
  const int d = (int)(i / kMfmaPW), e = (int)(i - (int64_t)d * kMfmaPW);
  const int g = d / kMfmaDims, w = d - g * kMfmaDims;
  double acc = 0.0;
  // entries k_mfma_dims never reads (tiles past NT, sq rows past n): not summed (half the reads
  // at n = 99, 8 of 16 tiles)
  if ((e >= a.NT * 256 && e < kMfmaNT * 256) || (e >= kMfmaNT * 256 + a.s.n && e < kMfmaNT * 256 + 256)) {
    red[i] = 0.0;
    return;
  }
  for (int r = 0; r < a.R; ++r) {
    const int id = ((r >> 3) * a.G + g) * 8 + (r & 7);   // inverse of k_conv_mfma's block map
    acc += partial[((int64_t)id * kMfmaDims + w) * kMfmaPW + e];
  }
  red[i] = acc;
}

// out in the conv layout of k_lag_dims (std, mean - S, (mean - S)^2, lags 1 .. nlag, lag n - 1)
__global__ __launch_bounds__(256) void k_mfma_dims(MfmaArgs a, const double* __restrict__ red, int nlag,
                                                   double* __restrict__ out) {
  const int D = a.s.D, n = a.s.n;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)(nlag + 4) * D) return;
  const int orow = (int)(i / D), d = (int)(i - (int64_t)orow * D);
  const double* rd = red + (int64_t)d * kMfmaPW;
  const double* sq = rd + kMfmaNT * 256;
  if (orow < 3) {
    out[i] = sq[256 + orow];
    return;
  }
  const int t = orow == nlag + 3 ? n - 1 : orow - 2;
  double v = 0.0;
  if (t >= 1 && t < n) {
    const int q = t >> 4, rr = t & 15;
    double c = 0.0;                               // C_t: tile 16 q (s <= r), tile 16 q - 16 (s > r)
    for (int sc = 0; sc <= rr; ++sc) c += rd[(q + 1) * 256 + (rr - sc) * 16 + sc];
    for (int sc = rr + 1; sc < 16; ++sc) c += rd[q * 256 + (rr + 16 - sc) * 16 + sc];
    double suf = 0.0, pre = 0.0;
    for (int r2 = t; r2 < n; ++r2) suf += sq[r2];
    for (int r2 = 0; r2 <= n - 1 - t; ++r2) pre += sq[r2];
    v = (suf + pre) - 2.0 * c;
  }
  out[i] = v;
}

// The matrix-core pass's geometry: ranges R (a multiple of 8) picked so that R x G workgroups (8 waves
// per CU at a time) end in as full a last round as possible, at least 4 rounds.
MfmaArgs mfma_args(const Src& s) {
  MfmaArgs a{};
  a.s = s;
  const int n = s.n;
  a.P = 32 * ((n + 46 - 8 + 31) / 32) + 8;
  a.PK = 4 * a.P + 16;
  a.NT = (n - 1) / 16 + 2;
  a.G = (s.D + kMfmaDims - 1) / kMfmaDims;
  const int64_t m2 = n_series(s);
  const int64_t groups = (m2 + 3) / 4;
  // workgroups resident at a time, as two per CU for every instance: the range count must not
  // depend on n, because diag_conv_work sizes the partials at n = kMfmaMinN for any n (a count
  // of 3 per CU below n = 113, following the small instance's occupancy, made a c3 pass at
  // n = 200 write past a work buffer sized at a different R)
  const int cus = device_cus() * 2;
  int best = 8;
  double best_eff = -1.0;
  for (int x = 1; x <= 64; ++x) {
    const int64_t R = 8 * x;
    if (R > groups) break;
    const int64_t wgs = R * a.G;
    const int64_t rounds = (wgs + cus - 1) / cus;
    double eff = (double)wgs / (double)(rounds * cus);
    if (rounds < 4) eff *= 0.5;                   // too few workgroups per CU to balance
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = (int)R;
    }
  }
  a.R = best;
  a.per = ((groups + a.R - 1) / a.R) * 4;
  return a;
}

// the samples, x0, the slack for the read-ahead past the last series, the sq rows
size_t mfma_lds(const MfmaArgs& a) {
  // k_conv_mfma<NTM <= 10> (n <= 144) keeps the sq rows in registers (no LDS for them) and
  // double-buffers the samples and x0 (PIPE)
  const bool small = a.s.n <= 16 * 9;
  const size_t buf = (size_t)(4 * a.PK + kMfmaSer);
  return ((small ? 2 : 1) * buf + kMfmaSlack + (small ? 0 : kMfmaSer * kSqStride)) * sizeof(double);
}

int64_t mfma_work(const MfmaArgs& a) {
  return (int64_t)a.R * a.G * kMfmaDims * kMfmaPW + (int64_t)a.s.D * kMfmaPW;
}

// k_conv_mfma<NTM>, the instance for 16 (NTM - 3) < n <= 16 (NTM - 1).  EDGE (NTM = 8: c4's halves; NTM = 14:
// c3's n = 200, E4 = 3): where n / 16 = NTM - 2 and 16 does not divide n the triangle is static (VT), with
// E4 = n % 16 / 4 + 1 row groups in the steps' last tiles (whole tiles from n % 16 = 12).
template <int NTM, bool EDGE>
void conv_mfma_instance(const MfmaArgs& a, double* partial, hipStream_t st) {
  auto go = [&](auto* kernel) { kernel<<<(unsigned)(a.R * a.G), kMfmaThreads, mfma_lds(a), st>>>(a, partial); };
  constexpr int VT = NTM - 2;
  const int n = a.s.n;
  if constexpr (EDGE) {
    if (n > 16 * VT && n < 16 * VT + 16) {
      switch ((n & 15) >> 2) {
        case 0: return go(k_conv_mfma<NTM, 1, VT>);
        case 1: return go(k_conv_mfma<NTM, 2, VT>);
        case 2: return go(k_conv_mfma<NTM, 3, VT>);
        default: return go(k_conv_mfma<NTM, 0, VT>);
      }
    }
  }
  go(k_conv_mfma<NTM>);
}

}  // namespace

// Stored split chains (halves 2) or completed halves of a streaming window that do not wrap
// (halves 1, wrap 0).  The staging's 32-bit lane offsets span a group's four series: two chains'
// rows (split chains) or four chains' (halves).
bool mfma_ok(const Src& s, int T) {
  const int64_t rows = (int64_t)s.n * s.sample_stride;
  const int64_t span = (s.halves == 2 ? 2 * s.chain_stride + 2 * rows : 3 * s.chain_stride + rows) + s.D;
  return (s.halves == 2 || s.halves == 1) && s.wrap == 0 && s.n >= kMfmaMinN && s.n <= kMfmaMaxN &&
         T >= s.n - 2 && n_series(s) >= 4 && s.chain_stride >= rows && span * 8 < kLagOOB;
}

// the matrix-core partials' bound that diag_conv_work reserves (the geometry at n = kMfmaMinN,
// either series layout): every launch checks its own geometry against it
int64_t mfma_work_bound(int64_t n_chains, int D) {
  int64_t w = 0;
  for (int halves = 1; halves <= 2; ++halves) {
    Src s{nullptr, 0, 0, 0, n_chains, kMfmaMinN, D, halves};
    w = std::max(w, mfma_work(mfma_args(s)));
  }
  return w;
}

hipError_t launch_conv_mfma(const Src& s, int nlag, double* work, double* out, hipStream_t st) {
  const MfmaArgs a = mfma_args(s);
  if (mfma_work(a) > mfma_work_bound(s.n_chains, s.D)) return hipErrorInvalidValue;   // never past the work
  double* partial = work;
  double* red = work + (int64_t)a.R * a.G * kMfmaDims * kMfmaPW;
  if (s.n <= 16 * 5) conv_mfma_instance<6, false>(a, partial, st);
  else if (s.n <= 16 * 7) conv_mfma_instance<8, true>(a, partial, st);
  else if (s.n <= 16 * 9) conv_mfma_instance<10, false>(a, partial, st);
  else if (s.n <= 16 * 11) conv_mfma_instance<12, false>(a, partial, st);
  else conv_mfma_instance<14, true>(a, partial, st);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t nr = (int64_t)s.D * kMfmaPW;
  k_mfma_ranges<<<(unsigned)((nr + 255) / 256), 256, 0, st>>>(a, partial, red);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t no = (int64_t)(nlag + 4) * s.D;
  k_mfma_dims<<<(unsigned)((no + 255) / 256), 256, 0, st>>>(a, red, nlag, out);
  return hipGetLastError();
}

}  // namespace hmc
