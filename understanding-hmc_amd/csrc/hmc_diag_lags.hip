// hmc_diag_lags.hip — the variogram lag sums and split-chain moments of convergence_stats (utils.py:88-126,
// :161-179) in ONE read of the samples, for any lag range: the VALU pass (k_conv_series, k_lag_classes, k_lag_dims)
// and the entry points behind hmc_convergence_sums, hmc_half_sums and hmc_variogram, which choose between it and
// the matrix-core pass of hmc_diag_mfma.hip.
//
// A *series* is one dimension d of one split chain j (n samples), flattened e = j*D + d; a wave
// owns 64 consecutive series (a tile: every lane busy whatever D; rows of a split chain are
// contiguous, so a wave's row load is one or two coalesced segments) and walks their n samples
// once.  Per series, with y = x - x_j[0] (shifted: well-conditioned sums),
//   V_t = sum_{s=t}^{n-1} (y_s - y_{s-t})^2 = 2 S2 - P(t) - Q(t) - 2 C_t,
//   C_t = sum_s y_s y_{s-t},  P(t) = sum_{s<t} y_s^2,  Q(t) = sum_{s>=n-t} y_s^2,
// so a lag costs ONE FMA per sample against a register ring of TL delayed samples.  A wave takes
// the TL lags t = gofs + 1 .. gofs + TL (lag group g: gofs = L0 + g*TL); its ring is fed by the
// sample stream delayed by gofs (the stream itself for gofs = 0).  Rows run in unrolled chunks of
// TL from row gofs, so ring slots are static registers:
//   * chunk 0 is the ramp: lag k of row i only meets the slots already written (k < i), so the
//     products with samples before the series start are never issued -- the pass costs the
//     triangle sum_t (n - t) of the reference's loop, not n*T -- and row i's running S2 is P(t);
//   * the delayed stream's squares over the run are P(n - gofs), from which Q(t) follows with the
//     ring's final contents (the last TL delayed samples);
//   * rows 0 .. gofs - 1 (lag groups with gofs > 0) only add their squares to S2.
// Lag group 0 of a first pass (L0 = 0) also sums the moments (mean_j: the samples added in order
// without FMA, NumPy's np.mean over axis 0 bit for bit; std_j (ddof 1) from S2 and s1) and the
// lag n - 1 the ESS loop reads last.
// Determinism: a wave owns the tiles tau = c + C (r + R i) of one class c (C = D / gcd(D, 64): lane
// l of every such tile holds dimension (64 c + l) mod D) and sums them in order in its lanes;
// k_lag_classes / k_lag_dims add the waves' lanes per dimension in a fixed order.  Wave ids are
// XCD-major (blocks b, b + 8, ... share an XCD): the lag groups of one (class, replica) run on the
// same XCD, so the rows one group reads are L2 hits for the others.
#include <algorithm>

#include "hmc_diag.hpp"

namespace hmc {

namespace {

#ifndef HMC_LAG_TL
#define HMC_LAG_TL 48
#endif
#ifndef HMC_LAG_PF
#define HMC_LAG_PF 16
#endif
// Lags per wave, rows in flight per stream and waves per SIMD.  One wave per SIMD with the whole
// register file, 48 lags (n = 50, the bench window, needs lags 1..48 + n - 1: one wave per tile) and
// 16 rows in flight measured best on the bench window (29 ms; 32 lags at two waves per SIMD: 65 ms,
// 53 ms with the ragged rows masked instead of branched; 48 lags at two waves per SIMD spill).
constexpr int kLagTL = HMC_LAG_TL;
constexpr int kLagPF = HMC_LAG_PF;   // divides kLagTL
// Tail lags: a first pass (mom) also sums the last `tail` <= kLagTail lags n - k, k = 1 .. tail, in
// difference form, V_{n-k} = sum_{i<k} (y_{n-k+i} - y_i)^2 (k terms each: rows 0 .. tail-1 and the
// last tail rows).  A complete pass then needs the lag groups only for lags 1 .. n - 1 - tail:
// n = 99 (c4's halves) takes two groups of 48 and a tail of 2 instead of a third group that would
// read every row again for one lag.
constexpr int kLagTail = 8;
// partial rows per wave: std, mean - S, (mean - S)^2, the tail lags n-1 .. n-kLagTail, the lag group
constexpr int kLagRows = kLagTL + 3 + kLagTail;
constexpr int kLagWaves = 8192;        // target waves per pass (4 rounds of 2 waves per SIMD)

struct LagArgs {
  Src s;
  int L0;          // lags L0 + 1 .. L0 + T (L0 a multiple of kLagPF)
  int T;           // lags of this pass (host geometry only)
  int G;           // lag groups, ceil(T / TL)
  int C, R;        // classes, replicas per class
  int mom;         // group 0 sums the moments and the tail lags (first pass)
  int tail;        // mom: tail lags n-1 .. n-tail (1 <= tail <= kLagTail)
  int64_t NT;      // tiles of 64 series
  int rowb;        // bytes between samples (sample_stride * 8)
};

__host__ __device__ inline int lag_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The tiles of one wave.  Z: the lag group starts at lag 1 (gofs = 0: the ring is fed by the
// stream itself; also the moments), else gofs > 0 (a second, delayed stream).  The two forms are
// separate instances, inlined into the two sides of k_conv_series' uniform branch, so that each
// keeps its own code (one body holding both forms spilled at 256 registers).
// WR: one series per chain in a circular window (Src::halves == 1, wrap > 0): sample s of every
// series sits in window row (slot0 + s) % wrap, so row offsets wrap (scalar arithmetic per load);
// the tile's buffer descriptor is based at the chain's window row 0.
template <int TL, int PF, bool Z, bool WR>
__device__ __forceinline__ void lag_wave(const LagArgs& a_, int W_, int g_, int c_, int r_, double* partial_) {
  // a function's arguments arrive in VGPRs: make every launch constant uniform again (SGPRs), so
  // that row and chunk tests stay scalar branches
  LagArgs a;
  a.s.x = uni(a_.s.x);
  a.s.chain_stride = uni(a_.s.chain_stride);
  a.s.sample_stride = uni(a_.s.sample_stride);
  a.s.base = uni(a_.s.base);
  a.s.n_chains = uni(a_.s.n_chains);
  a.s.n = uni(a_.s.n);
  a.s.D = uni(a_.s.D);
  a.s.halves = WR ? 1 : uni(a_.s.halves);
  a.s.wrap = WR ? uni(a_.s.wrap) : 0;
  a.s.slot0 = WR ? uni(a_.s.slot0) : 0;
  a.L0 = uni(a_.L0);
  a.G = uni(a_.G);
  a.C = uni(a_.C);
  a.R = uni(a_.R);
  a.mom = uni(a_.mom);
  a.tail = uni(a_.tail);
  a.NT = uni(a_.NT);
  a.rowb = uni(a_.rowb);
  const int W = uni(W_), g = uni(g_), c = uni(c_), r = uni(r_);
  double* const partial = uni(partial_);
  const int lane = threadIdx.x;
  const Src& s = a.s;
  const int n = s.n, D = s.D;
  const int gofs = a.L0 + g * TL;
  const bool mom = Z && a.mom;                     // wave-uniform (Z: gofs == 0, group 0)
  const int64_t m2 = n_series(s);
  // byte offset of sample `row` from a series' first window row (WR) or first sample
  auto rowoff = [&](int row) -> int {
    if constexpr (WR) {
      int p = row + s.slot0;
      p = p >= s.wrap ? p - s.wrap : p;
      return p * a.rowb;
    } else {
      return row * a.rowb;
    }
  };
  // lane -> (split chain jj past the tile's first, dim d): the same for every tile of the class
  const int per = 64 / lag_gcd(D, 64);             // split chains per class period (64 C / D)
  const int d0 = (int)((64 * (int64_t)c) % D);
  const int jj = (d0 + lane) / D;
  const int d = d0 + lane - jj * D;
  int64_t j0 = (64 * (int64_t)c) / D + (int64_t)per * r;
  const int64_t jstep = (int64_t)per * a.R;

  double v[TL];
#pragma unroll
  for (int k = 0; k < TL; ++k) v[k] = 0.0;
  double a_std = 0.0, a_m = 0.0, a_m2 = 0.0;
  double a_tail[kLagTail];
#pragma unroll
  for (int k = 0; k < kLagTail; ++k) a_tail[k] = 0.0;
  // shift of rows 1-2: the view's first sample
  const double Sd = s.x[s.base + (WR ? (int64_t)s.slot0 * s.sample_stride : 0) + d];
  if (gofs + 1 < n || mom) {
    // a tile's buffer descriptor and lane offset: split chain j0's first sample (wave-uniform) is the
    // base; lane offsets in bytes (host-checked below kLagOOB); lanes past the last series read
    // zeros (out of the buffer's range)
    auto tile_rsrc = [&](int64_t jt, int& vo) {
      const int64_t j = jt + jj;
      const double* tb = uni(split_ptr(s, jt, 0));
      vo = j < m2 ? (int)((split_ptr(s, j, 0) + d - tb) * 8) : kLagOOB + 64;
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(tb), 0, kLagOOB, 0x00020000);
    };
    // the first PF rows of the NEXT tile are loaded a whole tile ahead (a tile's first rows used to
    // wait a full memory latency: one wave per SIMD has nothing else to run meanwhile)
    double xn[PF];
    int voff_n = 0;
    __amdgpu_buffer_rsrc_t rs_n = tile_rsrc(j0, voff_n);
    const int64_t tau0 = c + (int64_t)a.C * r;
    if (tau0 < a.NT) {
#pragma unroll
      for (int p = 0; p < PF; ++p)
        xn[p] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs_n, voff_n, rowoff(p < n ? p : n - 1), 0));
    }
    for (int64_t tau = tau0; tau < a.NT; tau += (int64_t)a.C * a.R, j0 += jstep) {
      const bool valid = j0 + jj < m2;
      const __amdgpu_buffer_rsrc_t rs = rs_n;
      const int voff = voff_n;
      double xq[PF], xdq[PF];
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        xq[p] = xn[p];
        if constexpr (!Z) xdq[p] = xn[p];            // loop B's delayed rows 0 .. PF-1 (PF <= gofs)
      }
      if (tau + (int64_t)a.C * a.R < a.NT) {         // the next tile's first rows
        rs_n = tile_rsrc(j0 + jstep, voff_n);
#pragma unroll
        for (int p = 0; p < PF; ++p)
          xn[p] = __builtin_bit_cast(double,
                                     __builtin_amdgcn_raw_buffer_load_b64(rs_n, voff_n, rowoff(p < n ? p : n - 1), 0));
      }
      auto ldb = [&](int boff) -> double {         // sample at byte offset boff of the series
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, boff, 0));
      };
      auto ld = [&](int row) -> double { return ldb(rowoff(row)); };
      // the rolling prefetch's next row, as a running byte offset (a scalar the compiler may not
      // precompute per unrolled row: those products spilled the scalar file), clamped to row n - 1;
      // WR: a running row number, clamped, then wrapped (and the delayed stream's row wrapped apart)
      const int last_off = (n - 1) * a.rowb;
      const int dly_off = gofs * a.rowb;
      int nxt = PF * a.rowb;
      int nxr = PF;
      int dly_o = 0;                               // WR: the delayed row's offset of the last next_off()
      auto next_off = [&]() {
        if constexpr (WR) {
          int rw = nxr < n - 1 ? nxr : n - 1;
          asm volatile("" : "+s"(rw));
          ++nxr;
          asm volatile("" : "+s"(nxr));
          if constexpr (!Z) dly_o = rowoff(rw - gofs);
          return rowoff(rw);
        } else {
          int o = nxt < last_off ? nxt : last_off;
          asm volatile("" : "+s"(o));
          nxt += a.rowb;
          asm volatile("" : "+s"(nxt));
          return o;
        }
      };
      auto dly_of = [&](int o) -> int {            // offset of the delayed stream's row
        if constexpr (WR) return dly_o;
        else return o - dly_off;
      };
      const double sh = xq[0];                      // row 0
      const double sh2 = 2.0 * sh;
      double ring[TL];
#pragma unroll
      for (int k = 0; k < TL; ++k) ring[k] = 0.0;
      double s1 = 0.0, s2 = 0.0, r1 = 0.0, q4 = 0.0;
      if constexpr (!Z) {
        // rows 0 .. gofs - 1 (gofs >= PF, a multiple of PF): squares only; the rolling prefetch
        // runs on into loop B's first rows (slot = row % PF = (row - gofs) % PF)
        for (int s0 = 0; s0 < gofs; s0 += PF) {
#pragma unroll
          for (int p = 0; p < PF; ++p) {
            const double y = xq[p] - sh;
            s2 = __builtin_fma(y, y, s2);
            xq[p] = ldb(next_off());                 // row s0 + p + PF
          }
        }
      }
      const int nrow = n - gofs;                   // rows of loop B (>= 2)
      // TL rows from row gofs + ci TL.  FIRST: chunk 0 (ramp, P events); MOM: moments; DLY: the
      // delayed stream is a second load; RAG: fewer than TL rows left (uniform row tests)
      auto chunk = [&](auto first_c, auto mom_c, auto dly_c, auto rag_c, int ci) {
        constexpr bool FIRST = decltype(first_c)::value, MOM = decltype(mom_c)::value;
        constexpr bool DLY = decltype(dly_c)::value, RAG = decltype(rag_c)::value;
        const int s0 = gofs + ci * TL;
        const int rem = n - s0;
        auto row = [&](auto i_c) {
          constexpr int i = decltype(i_c)::value;
          // the loads are unconditional (rows past n re-read row n - 1): a load inside the ragged
          // rows' branch made its register a phi whose copy waited for vmcnt(0) every row
          const double x = xq[i % PF];
          const double xd = DLY ? xdq[i % PF] : x;
          {
            const int o = next_off();                // row min(s0 + i + PF, n - 1)
            xq[i % PF] = ldb(o);
            if (DLY) xdq[i % PF] = ldb(dly_of(o));
          }
          // ragged rows past n: a uniform branch over the arithmetic only (the loads above are
          // unconditional, so no load result is a phi: the waitcnt pass keeps its counts)
          if (!RAG || i < rem) {
            const double y = x - sh;
            if constexpr (MOM) {
              r1 += x;
              s1 += y;
            }
            s2 = __builtin_fma(y, y, s2);
#pragma unroll
            for (int k = 0; k < TL; ++k) {
              if (FIRST && k >= i) continue;       // the ramp: slot (i - 1 - k) not written yet
              v[k] = __builtin_fma(y, ring[(i - 1 - k + TL) % TL], v[k]);
            }
            if constexpr (FIRST) v[i] -= s2;       // P(gofs + 1 + i)
            const double rv = __builtin_fma(-2.0, xd, sh2);   // -2 (xd - sh): exact scaling
            if constexpr (DLY) q4 = __builtin_fma(rv, rv, q4);   // 4 x the delayed stream's squares
            ring[i] = rv;
          }
          // rows stay in program order: hoisting later rows' loads (the scheduler's choice in a
          // straight-line chunk) holds their results in registers and spills the ring
          __builtin_amdgcn_sched_barrier(0);
        };
        static_for<TL>(row);
      };
      auto run = [&](auto mom_c, auto dly_c) {
        if (nrow < TL) chunk(std::true_type{}, mom_c, dly_c, std::true_type{}, 0);
        else chunk(std::true_type{}, mom_c, dly_c, std::false_type{}, 0);
        int ci = 1;
        for (; (ci + 1) * TL <= nrow; ++ci) chunk(std::false_type{}, mom_c, dly_c, std::false_type{}, ci);
        if (ci * TL < nrow) chunk(std::false_type{}, mom_c, dly_c, std::true_type{}, ci);
      };
      if constexpr (Z) run(std::true_type{}, std::false_type{});   // (moments unused unless mom)
      else run(std::false_type{}, std::true_type{});
      // Q(t) = S2 - P(n - t), t = gofs + 1 + k: 4 (S2 - P(n - gofs)) (0 for gofs = 0), plus the
      // squares of the last k + 1 delayed samples, slot (n - 1 - gofs - k') mod TL, k' <= k
      double q = Z ? 0.0 : 4.0 * s2 - q4;
      const double s2x2 = 2.0 * s2;
      auto fin = [&](auto rl_c) {
        constexpr int RL = decltype(rl_c)::value;
#pragma unroll
        for (int k = 0; k < TL; ++k) {
          const double rk = ring[(RL - k + TL) % TL];
          q = __builtin_fma(rk, rk, q);            // 4 Q(gofs + 1 + k)
          v[k] += __builtin_fma(-0.25, q, s2x2);
        }
      };
      static_dispatch<TL>((n - 1 - gofs) % TL, fin);
      if (mom && valid) {
        const double dn = n;
        const double mean = r1 / dn;
        const double dm = mean - sh;
        const double mm2 = (s2 - 2.0 * dm * s1) + dn * (dm * dm);
        a_std += sqrt(mm2 > 0.0 ? mm2 / (dn - 1.0) : 0.0);
        const double e = mean - Sd;
        a_m += e;
        a_m2 = __builtin_fma(e, e, a_m2);
        // the tail lags n - k, k = 1 .. tail, in difference form: y_0 = 0 (the shift), y_1 .. y_{tail-1}
        // and the last tail samples, loaded together (clamped rows; unused values are masked)
        const int K = a.tail;
        double yl[kLagTail], yf[kLagTail];
#pragma unroll
        for (int j = 0; j < kLagTail; ++j) {
          const int rl = n - 1 - j;
          yl[j] = ld(j < K && rl > 0 ? rl : 0);     // y_{n-1-j} (+ sh)
          yf[j] = ld(j < K ? j : 0);               // y_j (+ sh)
        }
#pragma unroll
        for (int j = 0; j < kLagTail; ++j) {
          yl[j] -= sh;
          yf[j] -= sh;
        }
#pragma unroll
        for (int k = 1; k <= kLagTail; ++k) {
          if (k <= K) {                            // uniform
            // V_{n-k} = sum_{i<k} (y_{n-k+i} - y_i)^2, y_{n-k+i} = yl[k-1-i]
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < k; ++i) {
              const double df = yl[k - 1 - i] - yf[i];
              acc = __builtin_fma(df, df, acc);
            }
            a_tail[k - 1] += acc;
          }
        }
      }
    }
  }
  double* out = partial + (int64_t)W * kLagRows * 64 + lane;
  out[0] = a_std;
  out[64] = a_m;
  out[128] = a_m2;
#pragma unroll
  for (int k = 0; k < kLagTail; ++k) out[(3 + k) * 64] = a_tail[k];
#pragma unroll
  for (int k = 0; k < TL; ++k) out[(3 + kLagTail + k) * 64] = v[k];
}

template <int TL, int PF, bool WR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv_series(LagArgs a, double* partial) {
  const int W = blockIdx.x;
  const int u = W >> 3;
  const int g = u % a.G;
  const int cr = (u / a.G) * 8 + (W & 7);
  const int c = cr % a.C, r = cr / a.C;
  if (r >= a.R) return;                            // grid padding (never reduced)
  if (a.L0 + g * TL == 0) lag_wave<TL, PF, true, WR>(a, W, g, c, r, partial);
  else lag_wave<TL, PF, false, WR>(a, W, g, c, r, partial);
}

// inter[(c * G + g) * kLagRows + row][l] = sum over the replicas r (in order) of the waves' lanes
__global__ __launch_bounds__(256) void k_lag_classes(LagArgs a, const double* __restrict__ partial,
                                                     double* __restrict__ inter) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tot = (int64_t)a.C * a.G * kLagRows * 64;
  if (i >= tot) return;
  const int l = (int)(i & 63);
  const int64_t cgr = i >> 6;
  const int row = (int)(cgr % kLagRows);
  const int64_t cg = cgr / kLagRows;
  const int g = (int)(cg % a.G), c = (int)(cg / a.G);
  double acc = 0.0;
  for (int r = 0; r < a.R; ++r) {
    const int cr = r * a.C + c;
    const int64_t W = 8 * (g + (int64_t)a.G * (cr / 8)) + (cr & 7);
    acc += partial[(W * kLagRows + row) * 64 + l];
  }
  inter[i] = acc;
}

// out[orow][d]: conv layout (conv != 0: rows std, mean - S, (mean - S)^2, lags L0 + 1 + skip ..,
// lag n - 1; nlag lags) or lags only; lags t >= n are 0.  Sums the classes' lanes that hold
// dimension d, in a fixed order.
__global__ __launch_bounds__(256) void k_lag_dims(LagArgs a, const double* __restrict__ inter, int conv, int skip,
                                                  int nlag, double* __restrict__ out) {
  const int D = a.s.D;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nrow = conv ? nlag + 4 : nlag;
  if (i >= (int64_t)nrow * D) return;
  const int orow = (int)(i / D), d = (int)(i - (int64_t)orow * D);
  int g = 0, prow;
  int t = 0;                                       // lag (0: a moment row)
  if (conv && orow < 3) prow = orow;
  else {
    t = (conv && orow == nlag + 3) ? a.s.n - 1 : a.L0 + 1 + skip + orow - (conv ? 3 : 0);
    if (a.mom && t >= a.s.n - a.tail) {            // a tail lag (difference form, group 0)
      prow = 3 + (a.s.n - 1 - t);
    } else {
      const int k = t - a.L0 - 1;                  // lag index inside the pass
      g = k / kLagTL;
      prow = 3 + kLagTail + k % kLagTL;
    }
  }
  double acc = 0.0;
  if (t < a.s.n && t >= 0 && g < a.G && !(conv && orow == nlag + 3 && a.s.n < 2)) {
    for (int c = 0; c < a.C; ++c) {
      int l = (int)(((int64_t)d - 64 * (int64_t)c) % D);
      if (l < 0) l += D;
      for (; l < 64; l += D) acc += inter[(((int64_t)c * a.G + g) * kLagRows + prow) * 64 + l];
    }
  }
  out[i] = acc;
}

// G lag groups (and the tail) of a pass over lags L0 + 1 .. L0 + T.  A first pass (mom) asking for
// every lag (T >= n - 2; lag n - 1 always comes from the tail) runs the groups up to lag
// n - 1 - tail only and sums the rest, tail <= kLagTail lags, in difference form.
LagArgs lag_args(const Src& s, int L0, int T, int mom) {
  LagArgs a{};
  a.s = s;
  a.L0 = L0;
  a.T = T;
  a.G = (T + kLagTL - 1) / kLagTL;
  a.mom = mom;
  a.tail = mom ? 1 : 0;
  if (mom && L0 == 0 && T >= s.n - 2 && s.n >= 2) {
    const int need = s.n - 1 - kLagTail;           // lags the groups must cover at least
    const int G = need > 0 ? (need + kLagTL - 1) / kLagTL : 1;
    const int Tg = std::min(G * kLagTL, s.n - 2);
    a.G = G;
    a.T = Tg > 0 ? Tg : 0;
    a.tail = s.n - 1 - a.T;
  }
  a.C = s.D / lag_gcd(s.D, 64);
  a.NT = (n_series(s) * (int64_t)s.D + 63) / 64;
  const int64_t per_class = (a.NT + a.C - 1) / a.C;
  const int64_t R = (kLagWaves + (int64_t)a.C * a.G - 1) / ((int64_t)a.C * a.G);
  a.R = (int)(R < per_class ? (R < 1 ? 1 : R) : per_class);
  a.rowb = (int)(s.sample_stride * 8);
  return a;
}

int64_t lag_grid(const LagArgs& a) { return 8 * (int64_t)a.G * (((int64_t)a.C * a.R + 7) / 8); }
int64_t lag_work(const LagArgs& a) {
  return lag_grid(a) * kLagRows * 64 + (int64_t)a.C * a.G * kLagRows * 64;
}

// Work (doubles) that any pass of at most T lags (L0 = 0, n unknown: a complete first pass may take
// fewer groups than ceil(T / TL)) over n_chains chains of D dims needs: the largest over the group
// counts it could run.
int64_t lag_work_bound(int64_t n_chains, int D, int T, int mom) {
  int64_t w = 0;
  const int Gmax = (T + kLagTL - 1) / kLagTL;
  for (int G = 1; G <= Gmax; ++G) {
    Src s{nullptr, 0, 0, 0, n_chains, 2, D};
    LagArgs a = lag_args(s, 0, G * kLagTL, 0);   // geometry of G groups (pairs: the most series)
    a.mom = mom;
    w = std::max(w, lag_work(a));
  }
  return w;
}

// One read of the samples: lags L0 + 1 .. L0 + T (group 0 also the moments when mom), reduced into
// out (conv layout or lags only, from lag L0 + 1 + skip, nlag lags).
// Lane offsets (bytes from a tile's first series) and row offsets must stay inside the buffer
// bound kLagOOB (1 GiB): a tile spans at most 64 / D + 2 series; the second half of a chain starts
// n * sample_stride after its first (chain_stride >= that for every q_chain view).  So one chain's
// samples (its stride) must stay well within 1 GiB: e.g. D = 1000 up to ~40,000 stored samples per
// chain, D = 100 up to ~400,000 (hmc_amd.diagnostics splits larger views by dimension).
bool lag_view_ok(const Src& s) {
  const int64_t cs = s.chain_stride, ss = s.sample_stride;
  if (ss < 1 || ss * 8 > 0x7FFFFFFF || s.D < 1) return false;
  if (s.halves == 2) {
    if (cs < (int64_t)s.n * ss) return false;
    const int64_t span = ((64 / s.D + 2) / 2 + 1) * cs + (int64_t)s.n * ss + s.D;   // doubles
    return (span + (int64_t)s.n * ss) * 8 < kLagOOB;
  }
  // one series per chain: a tile spans at most 64 / D + 2 chains; rows up to the window's last
  const bool wr = s.wrap > 0;
  const int64_t rows = wr ? (int64_t)s.wrap : (int64_t)s.n;
  if (wr && (s.slot0 < 0 || s.slot0 >= s.wrap || s.n > s.wrap)) return false;
  const int64_t span = (64 / s.D + 2) * cs + s.D;
  return (span + rows * ss) * 8 < kLagOOB;
}

hipError_t launch_lags(const Src& s, int L0, int T, int mom, int conv, int skip, int nlag, double* work, double* out,
                       hipStream_t st) {
  if (T < 1 || L0 < 0 || L0 % kLagPF != 0) return hipErrorInvalidValue;
  if (!lag_view_ok(s)) return hipErrorInvalidValue;
  const bool wr = s.halves == 1 && s.wrap > 0;
  const LagArgs a = lag_args(s, L0, T, mom);
  const int64_t grid = lag_grid(a);
  double* partial = work;
  double* inter = work + grid * kLagRows * 64;
  if (wr) k_conv_series<kLagTL, kLagPF, true><<<(unsigned)grid, 64, 0, st>>>(a, partial);
  else k_conv_series<kLagTL, kLagPF, false><<<(unsigned)grid, 64, 0, st>>>(a, partial);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t ni = (int64_t)a.C * a.G * kLagRows * 64;
  k_lag_classes<<<(unsigned)((ni + 255) / 256), 256, 0, st>>>(a, partial, inter);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t no = (int64_t)(conv ? nlag + 4 : nlag) * s.D;
  k_lag_dims<<<(unsigned)((no + 255) / 256), 256, 0, st>>>(a, inter, conv, skip, nlag, out);
  return hipGetLastError();
}

// A complete first pass (moments, every lag): the matrix cores where they take the view
// (HMC_LAG_NO_MFMA forces the VALU pass for an A/B run).
hipError_t launch_complete(const Src& s, int T, double* work, double* out, hipStream_t st) {
#ifndef HMC_LAG_NO_MFMA
  if (mfma_ok(s, T)) return launch_conv_mfma(s, T, work, out, st);
#endif
  return launch_lags(s, 0, T, 1, 1, 0, T, work, out, st);
}

}  // namespace

bool diag_view_ok(int64_t n_chains, int64_t cs, int64_t ss, int n, int D, int halves, int wrap, int slot0) {
  Src s{nullptr, cs, ss, 0, n_chains, n, D, halves, wrap, slot0};
  return lag_view_ok(s);
}

int64_t diag_variogram_work(int64_t n_chains, int D, int nlags) {
  Src s{nullptr, 0, 0, 0, n_chains, 2, D};
  return lag_work(lag_args(s, 0, nlags + kLagPF - 1, 0));   // the lag range may start up to PF-1 lower
}

int64_t diag_conv_work(int64_t n_chains, int D, int T) {
  int64_t w = lag_work_bound(n_chains, D, T, 1);
  // a complete pass of split chains of kMfmaMinN .. T + 2 samples may take the matrix cores (their
  // geometry depends on the chains and dims only)
  if (T + 2 >= kMfmaMinN) w = std::max(w, mfma_work_bound(n_chains, D));   // stored split chains or halves
  return w;
}

hipError_t launch_conv_fused(const double* x, int64_t n_chains, int64_t cs, int64_t ss, int64_t base, int n, int D,
                             int T, double* work, double* out, hipStream_t st) {
  Src s{x, cs, ss, base, n_chains, n, D};
  return launch_complete(s, T, work, out, st);
}

hipError_t launch_half_sums(const double* x, int64_t n_chains, int64_t cs, int64_t ss, int D, int wrap, int slot0,
                            int n, int T, double* work, double* out, hipStream_t st) {
  // a half that does not reach the window's end reads plain strided rows (no per-row wrap)
  if (wrap > 0 && slot0 + n <= wrap) wrap = 0;
  Src s{x, cs, ss, 0, n_chains, n, D, 1, wrap, slot0};
  if (wrap <= 0) s.base = (int64_t)slot0 * ss;   // no wrap: sample s in row slot0 + s
  return launch_complete(s, T, work, out, st);
}

hipError_t launch_variogram(const double* x, int64_t n_chains, int64_t cs, int64_t ss, int64_t base, int n, int D,
                            int t0, int t1, double* work, double* out, hipStream_t st) {
  Src s{x, cs, ss, base, n_chains, n, D};
  const int L0 = (t0 - 1) / kLagPF * kLagPF;   // the pass starts at a prefetch-aligned lag
  return launch_lags(s, L0, t1 - 1 - L0, 0, 0, t0 - 1 - L0, t1 - t0, work, out, st);
}

}  // namespace hmc
