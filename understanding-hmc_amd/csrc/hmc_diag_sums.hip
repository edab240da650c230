// hmc_diag_sums.hip — the elementwise pieces of the diagnostics: per-split-chain moments (k_split_moments)
// and deterministic two-stage sums over rows (k_rowsum_partial + k_colsum), behind hmc_split_moments and
// hmc_rowsum; k_colsum also closes the streaming pass (hmc_diag_stream.hip).
#include "hmc_diag.hpp"

namespace hmc {

namespace {

constexpr int kRowChunk = 256;   // rows per partial-sum block

// One thread per (split chain j, dim d): two-pass mean and std (ddof = 1, numpy np.std(ddof=1)).
__global__ __launch_bounds__(256) void k_split_moments(Src s, double* mean_out, double* std_out) {
  const int d = blockIdx.y * kDimTile + (threadIdx.x & (kDimTile - 1));
  const int64_t j = (int64_t)blockIdx.x * (256 / kDimTile) + (threadIdx.x / kDimTile);
  if (d >= s.D || j >= 2 * s.n_chains) return;
  double sum = 0.0;
  for (int t = 0; t < s.n; ++t) sum += split_ptr(s, j, t)[d];
  const double mean = sum / s.n;
  double m2 = 0.0;
  for (int t = 0; t < s.n; ++t) {
    const double e = split_ptr(s, j, t)[d] - mean;
    m2 += e * e;
  }
  mean_out[j * s.D + d] = mean;
  std_out[j * s.D + d] = sqrt(m2 / (s.n - 1));
}

struct Rows {
  const double* x;
  int64_t n_outer, outer_stride, n_inner, inner_stride, base;
  int D;
  const double* center;  // null: plain sum; else sum of (x - center_d)^2
};

// partial[chunk][d] = sum over the chunk's rows.  Block = 4 row-lanes x 64 dims.
__global__ __launch_bounds__(256) void k_rowsum_partial(Rows r, double* partial) {
  __shared__ double red[4][kDimTile];
  const int dl = threadIdx.x & (kDimTile - 1);
  const int rl = threadIdx.x / kDimTile;
  const int d = blockIdx.y * kDimTile + dl;
  const int64_t rows = r.n_outer * r.n_inner;
  const int64_t r0 = (int64_t)blockIdx.x * kRowChunk;
  double acc = 0.0;
  if (d < r.D) {
    const double c = r.center ? r.center[d] : 0.0;
    for (int i = rl; i < kRowChunk; i += 4) {
      const int64_t row = r0 + i;
      if (row >= rows) break;
      const int64_t o = row / r.n_inner, in = row - o * r.n_inner;
      const double v = r.x[r.base + o * r.outer_stride + in * r.inner_stride + d];
      if (r.center) {
        const double e = v - c;
        acc += e * e;
      } else {
        acc += v;
      }
    }
  }
  const double sum = block_sum4(red, rl, dl, acc);
  if (rl == 0 && d < r.D) partial[(int64_t)blockIdx.x * r.D + d] = sum;
}

// out[c] = sum_k partial[k][c] for c < ncols (fixed order: deterministic); ACC: out[c] += it
// (accumulates across calls).
template <bool ACC>
__global__ __launch_bounds__(256) void k_colsum(const double* partial, int64_t nchunks, int64_t ncols, double* out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  double acc = 0.0;
  for (int64_t k = 0; k < nchunks; ++k) acc += partial[k * ncols + c];
  if constexpr (ACC) out[c] += acc;
  else out[c] = acc;
}

int64_t rows_chunks(int64_t rows) { return (rows + kRowChunk - 1) / kRowChunk; }

}  // namespace

hipError_t launch_colsum(const double* partial, int64_t nchunks, int64_t ncols, double* out, bool accumulate,
                         hipStream_t st) {
  const unsigned grid = (unsigned)((ncols + 255) / 256);
  if (accumulate) k_colsum<true><<<grid, 256, 0, st>>>(partial, nchunks, ncols, out);
  else k_colsum<false><<<grid, 256, 0, st>>>(partial, nchunks, ncols, out);
  return hipGetLastError();
}

int64_t diag_rowsum_work(int64_t rows, int D) { return rows_chunks(rows) * D; }

hipError_t launch_split_moments(const double* x, int64_t n_chains, int64_t cs, int64_t ss, int64_t base, int n,
                                int D, double* mean_out, double* std_out, hipStream_t st) {
  Src s{x, cs, ss, base, n_chains, n, D};
  const int64_t m2 = 2 * n_chains;
  dim3 grid((unsigned)((m2 + 3) / 4), (unsigned)((D + kDimTile - 1) / kDimTile));
  k_split_moments<<<grid, 256, 0, st>>>(s, mean_out, std_out);
  return hipGetLastError();
}

hipError_t launch_rowsum(const double* x, int64_t n_outer, int64_t os, int64_t n_inner, int64_t is, int64_t base,
                         int D, const double* center, double* work, double* out, hipStream_t st) {
  Rows r{x, n_outer, os, n_inner, is, base, D, center};
  const int64_t nch = rows_chunks(n_outer * n_inner);
  dim3 grid((unsigned)nch, (unsigned)((D + kDimTile - 1) / kDimTile));
  k_rowsum_partial<<<grid, 256, 0, st>>>(r, work);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_colsum(work, nch, D, out, false, st);
}

}  // namespace hmc
