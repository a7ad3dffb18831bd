// Held-out evaluation behind the scoring kernels: the (margin, label) pairs of
// a scored batch reduced into the metric accumulators of
// twitter_stream_ml_amd/models/metrics.py.
//
//   margin  pred[k] of scored row k (launch_score with kLinkMargin)
//   label   retweetCount of raw row rows[k] (k when rows is null), scalar
//           column 0 of the raw slot
//
// One thread per scored row, grid-stride.  Every integer accumulator is an
// integer sum, so it is the same whatever the order:
//   k_eval_binary      hist[2][kEvalBins] in LDS (uint32, non-returning adds),
//                      flushed to the int64 global histogram for its non-zero
//                      bins only; n, n_nan and the confusion counts from
//                      ballots, one LDS add per wave, one global add per
//                      workgroup and word
//   k_eval_regression  n, n_nan the same way
// The fp64 sums take a fixed order: a thread adds its rows in grid-stride
// order, a wave combines with the xor-shuffle tree, the wave sums are added
// in wave order into one partial per workgroup, and k_eval_final (one
// workgroup) adds the partials in index order.  The grid depends on n_raw
// alone, so a batch's sums depend on the batch alone.
//
// Every per-row term is a fixed sequence of IEEE operations (contraction off:
// no fused multiply-add, no libm), so the host forms the same bits
// (metrics.py log1p_exp_neg, regression_terms).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

// No contraction in this file.  The build's -ffp-contract=fast disregards the
// pragma, so _build.py also compiles this file with -ffp-contract=off.
#pragma clang fp contract(off)

namespace twtml {

namespace {

// metrics.py margin_bin (m is not NaN)
__device__ __forceinline__ int eval_margin_bin(double m) {
  const uint64_t u = __builtin_bit_cast(uint64_t, m);
  const int e = int((u >> 52) & 0x7ff) - 1023;
  const int f = int((u >> 46) & 0x3f);
  const int mag = e < -20 ? 0 : (e >= 12 ? 2048 : (e + 20) * 64 + f + 1);
  return (u >> 63) ? 2048 - mag : 2048 + mag;
}

// metrics.py log1p_exp_neg: log1p(exp(-a)), a >= 0
__device__ __forceinline__ double eval_log1p_exp_neg(double a) {
  constexpr double kLog2e = 0x1.71547652b82fep+0;
  constexpr double kLn2Hi = 0x1.62e42fee00000p-1;
  constexpr double kLn2Lo = 0x1.a39ef35793c76p-33;
  if (a > 700.0) return 0.0;
  const double k = floor(a * kLog2e + 0.5);
  const double r = (k * kLn2Hi - a) + k * kLn2Lo;
  double p = 1.0 + r * (1.0 / 14);
#pragma unroll
  for (int j = 13; j > 1; --j) p = 1.0 + (r * (1.0 / j)) * p;
  p = 1.0 + r * p;
  const double t = p * __builtin_bit_cast(double, uint64_t(1023 - int(k)) << 52);   // 2^-k, k <= 1010
  const double s = t / (2.0 + t);
  const double s2 = s * s;
  double q = 1.0 / 37;
#pragma unroll
  for (int d = 35; d > 1; d -= 2) q = 1.0 / d + s2 * q;
  q = 1.0 + s2 * q;
  return 2.0 * (s * q);
}

// Scored rows: the device count, never beyond the raw batch.
__device__ __forceinline__ int64_t eval_rows(const DevRawBatch& b, const int64_t* counters) {
  const int64_t n = counters[0];
  return n < 0 ? 0 : (n > b.n ? b.n : n);
}

// Scored row k of the wave's lane: margin and raw row id; false beyond n (or
// for a row id outside the batch, which the host's count check reports).
__device__ __forceinline__ bool eval_load(const DevRawBatch& b, const double* pred, const int64_t* rows, int64_t k,
                                          int64_t n, double* m, int64_t* row) {
  if (k >= n) return false;
  *m = pred[k];
  *row = rows ? rows[k] : k;
  return uint64_t(*row) < uint64_t(b.n);
}

__device__ __forceinline__ uint32_t count_of(bool v) { return uint32_t(__popcll(__ballot(v))); }

// wave sums in wave order (after the caller's __syncthreads)
__device__ __forceinline__ double wave_order_sum(const double* w) {
  double s = w[0];
#pragma unroll
  for (int i = 1; i < kBlock / kWave; ++i) s += w[i];
  return s;
}

__global__ __launch_bounds__(kBlock) void k_eval_binary(DevRawBatch b, const double* pred, const int64_t* rows,
                                                        const int64_t* counters, int64_t label_threshold,
                                                        double logit_thr, int64_t* out_i, double* partials) {
  __shared__ uint32_t hist[2 * kEvalBins];
  __shared__ uint32_t cnt[kEvalIntHead];
  __shared__ double wsum[kBlock / kWave];
  for (int i = threadIdx.x; i < 2 * kEvalBins; i += kBlock) hist[i] = 0;
  if (threadIdx.x < kEvalIntHead) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t n = eval_rows(b, counters);
  const int lane = lane_id();
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  uint32_t c_n = 0, c_nan = 0, c_tn = 0, c_fp = 0, c_fn = 0, c_tp = 0;   // wave-uniform
  double loss = 0.0;
  for (int64_t k0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); k0 < n; k0 += stride) {
    double m = 0.0;
    int64_t row = 0;
    const bool active = eval_load(b, pred, rows, k0 + lane, n, &m, &row);
    const bool nan = m != m;
    const bool ok = active && !nan;
    const bool lab = ok && raw_scalar(b, 0, row) >= label_threshold;
    const bool pos = m > logit_thr;
    c_nan += count_of(active && nan);
    c_n += count_of(ok);
    c_tn += count_of(ok && !lab && !pos);
    c_fp += count_of(ok && !lab && pos);
    c_fn += count_of(ok && lab && !pos);
    c_tp += count_of(ok && lab && pos);
    if (ok) {
      atomicAdd(&hist[(lab ? kEvalBins : 0) + eval_margin_bin(m)], 1u);
      const double hinge = lab ? -m : m;
      loss += (hinge > 0.0 ? hinge : 0.0) + eval_log1p_exp_neg(fabs(m));
    }
  }
  loss = wave_sum(loss);
  if (lane == 0) {
    wsum[threadIdx.x / kWave] = loss;
    atomicAdd(&cnt[kEvalN], c_n);
    atomicAdd(&cnt[kEvalNan], c_nan);
    atomicAdd(&cnt[kEvalConf + 0], c_tn);
    atomicAdd(&cnt[kEvalConf + 1], c_fp);
    atomicAdd(&cnt[kEvalConf + 2], c_fn);
    atomicAdd(&cnt[kEvalConf + 3], c_tp);
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(out_i);
  for (int i = threadIdx.x; i < 2 * kEvalBins; i += kBlock) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(&out[kEvalIntHead + i], (unsigned long long)v);
  }
  if (threadIdx.x < kEvalIntHead) {
    const uint32_t v = cnt[threadIdx.x];
    if (v) atomicAdd(&out[threadIdx.x], (unsigned long long)v);
  }
  if (threadIdx.x == 0) partials[int64_t(blockIdx.x) * kEvalF64Words] = wave_order_sum(wsum);
}

__global__ __launch_bounds__(kBlock) void k_eval_regression(DevRawBatch b, const double* pred, const int64_t* rows,
                                                            const int64_t* counters, int64_t* out_i,
                                                            double* partials) {
  constexpr int kSums = 6;   // y, y^2, p, p^2, (y - p)^2, |y - p|
  __shared__ uint32_t cnt[kEvalIntHead];
  __shared__ double wsum[kSums][kBlock / kWave];
  if (threadIdx.x < kEvalIntHead) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t n = eval_rows(b, counters);
  const int lane = lane_id();
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  uint32_t c_n = 0, c_nan = 0;
  double sy = 0.0, sy2 = 0.0, sp = 0.0, sp2 = 0.0, se2 = 0.0, sae = 0.0;
  for (int64_t k0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); k0 < n; k0 += stride) {
    double p = 0.0;
    int64_t row = 0;
    const bool active = eval_load(b, pred, rows, k0 + lane, n, &p, &row);
    const bool nan = p != p;
    const bool ok = active && !nan;
    c_nan += count_of(active && nan);
    c_n += count_of(ok);
    if (ok) {
      const double y = double(raw_scalar(b, 0, row));
      const double e = y - p;
      sy += y;
      sy2 += y * y;
      sp += p;
      sp2 += p * p;
      se2 += e * e;
      sae += fabs(e);
    }
  }
  const double sums[kSums] = {wave_sum(sy), wave_sum(sy2), wave_sum(sp), wave_sum(sp2), wave_sum(se2), wave_sum(sae)};
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) wsum[j][threadIdx.x / kWave] = sums[j];
    atomicAdd(&cnt[kEvalN], c_n);
    atomicAdd(&cnt[kEvalNan], c_nan);
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(out_i);
  if (threadIdx.x < kEvalIntHead) {
    const uint32_t v = cnt[threadIdx.x];
    if (v) atomicAdd(&out[threadIdx.x], (unsigned long long)v);
  }
  if (threadIdx.x < kSums) partials[int64_t(blockIdx.x) * kEvalF64Words + threadIdx.x] = wave_order_sum(wsum[threadIdx.x]);
}

// out_d[j] = partials[0][j] + partials[1][j] + ... in index order (columns
// >= nd: 0); the scored-row count goes along with the accumulator.  The
// partials are staged in LDS by the whole workgroup first: a lane adding 256
// dependent global loads took longer than the reduction kernel itself.
__global__ __launch_bounds__(kBlock) void k_eval_final(const double* partials, int np, int nd, double* out_d,
                                                       const int64_t* counters, int64_t* out_i) {
  __shared__ double part[kEvalMaxGrid * kEvalF64Words];
  const int total = np * kEvalF64Words;   // np <= kEvalMaxGrid
  for (int i = threadIdx.x; i < total; i += kBlock) part[i] = partials[i];
  __syncthreads();
  const int j = threadIdx.x;
  if (j == 0) out_i[kEvalScored] = counters[0];
  if (j >= kEvalF64Words) return;
  double s = 0.0;
  if (j < nd)
    for (int i = 0; i < np; ++i) s += part[i * kEvalF64Words + j];
  out_d[j] = s;
}

}  // namespace

int eval_grid(int64_t n_raw) {
  const int g = ceil_div(n_raw, kBlock);
  return g < 1 ? 1 : (g > kEvalMaxGrid ? kEvalMaxGrid : g);
}

void launch_eval(const DevRawBatch& b, const double* pred, const int64_t* rows, const int64_t* counters,
                 int64_t label_threshold, double logit_thr, int64_t* out_i, double* out_d, double* partials,
                 hipStream_t s) {
  TWTML_HIP_CHECK(hipMemsetAsync(out_i, 0, sizeof(int64_t) * kEvalIntWords, s));
  const int grid = eval_grid(b.n);
  if (label_threshold >= 0) {
    TWTML_LAUNCH(k_eval_binary, dim3(grid), dim3(kBlock), 0, s, b, pred, rows, counters, label_threshold, logit_thr,
                 out_i, partials);
    TWTML_LAUNCH(k_eval_final, dim3(1), dim3(kBlock), 0, s, partials, grid, 1, out_d, counters, out_i);
  } else {
    TWTML_LAUNCH(k_eval_regression, dim3(grid), dim3(kBlock), 0, s, b, pred, rows, counters, out_i, partials);
    TWTML_LAUNCH(k_eval_final, dim3(1), dim3(kBlock), 0, s, partials, grid, 6, out_d, counters, out_i);
  }
}

}  // namespace twtml
