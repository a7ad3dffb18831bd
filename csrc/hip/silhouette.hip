// Silhouette of a k-means model on one batch (MLlib ClusteringEvaluator,
// squared Euclidean; the contract is models/silhouette.py), for gfx950.
//
// The engine has assigned the rows (labels, sizes) and produced the batch's
// cluster means in fp64 and dev2_p = |x_p - mu_A(p)|^2 with the cost kernel.
// This file adds
//
//   k_sil_means     mean = sums / counts
//   k_sil_wmax      per-cluster max of dev2, integer atomic max on the bits
//   k_sil_wsum      per-cluster int64 sum of rint(dev2 2^(40 - e)): the same
//                   bits in any order, no float atomics
//   k_sil_stats     W, V = W / N, the fp32 means and B = |mu|^2 + V
//   k_sil_neighbor_{mfma,scalar}
//                   per row the closest other cluster by mean distance, then
//                   a, b, s and the batch's integer words
//
// The neighbour pass is an assignment-shaped n x k x d sweep of the fp32 score
// B_G - 2 x.mu_G (= D(x, G) - |x|^2).  On the matrix cores it uses
// v_mfma_f32_32x32x2f32, 32 clusters x 32 points per wave, not the bf16 hi/lo
// split of the assign kernels: the split's ~3 * 2^-18 relative product error
// is above the fp32 dot-product bound 2 (dp + 4) 2^-24 (|x|^2 + |mu|^2 + V)
// that the candidates are chosen under for dp < 128, and no refine list
// settles near ties afterwards -- the fp64 finish looks at two candidates
// only.  For the same reason a lane keeps its three smallest scores as exact
// (value, index) pairs, not as keys with the index packed into the mantissa
// (2^(lbits - 23) relative, again above the bound).  Among three, at least two
// are not the row's own cluster.
//
// Finish in fp64: for the (at most two) best candidates G != A(p), D(x_p, G) =
// sum_j (double(X[p][j]) f64[j] - mu_G[j])^2 + V_G with k_km_cost's term
// (explicit fma), one lane per candidate adding its columns in column order:
// a row's bits depend on the row and the cluster statistics alone.  b is the
// smaller (lower index on an exact tie), so b is exactly the fp64 value of the
// neighbour it names.  a = (N dev2 + W) / (N - 1) and the three-branch s are
// single IEEE operations (this file is compiled with -ffp-contract=off).
// rint(s 2^36) and the row go to workgroup-private LDS histograms (k <=
// kSilLdsBins), flushed with 64-bit integer atomics, else straight to global
// 64-bit integer atomics; singletons are counted from ballots.
#include "silhouette.h"

#include <cfloat>
#include <cmath>

#include "common.h"

namespace twtml {

constexpr int kSilLdsBins = 1024;   // k up to which the words are privatised in LDS (16 KB)

__device__ __forceinline__ int sil_label(int lab, int k) { return lab < 0 ? 0 : (lab < k ? lab : k - 1); }

__global__ void k_sil_means(const double* sums, const double* counts, int k, int d, double* mean) {
  const int64_t total = int64_t(k) * d;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * blockDim.x) {
    const double c = counts[i / d];
    mean[i] = c > 0.0 ? sums[i] / c : 0.0;
  }
}

void launch_sil_means(const double* sums, const double* counts, int k, int d, double* mean, hipStream_t s) {
  int grid = int((int64_t(k) * d + kBlock - 1) / kBlock);
  if (grid > 8192) grid = 8192;
  TWTML_LAUNCH(k_sil_means, dim3(grid), dim3(kBlock), 0, s, sums, counts, k, d, mean);
}

// dev2 >= 0: the order of the bit patterns is the order of the values
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_sil_wmax(const double* dev2, const int32_t* labels, int64_t n, int k,
                                                     unsigned long long* wmax) {
  extern __shared__ unsigned long long lw[];
  if (LDS) {
    for (int c = threadIdx.x; c < k; c += kBlock) lw[c] = 0ull;
    __syncthreads();
  }
  unsigned long long* dst = LDS ? lw : wmax;
  for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < n; p += int64_t(gridDim.x) * kBlock)
    atomicMax(&dst[sil_label(labels[p], k)], static_cast<unsigned long long>(__double_as_longlong(dev2[p])));
  if (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kBlock)
      if (lw[c]) atomicMax(&wmax[c], lw[c]);
  }
}

// the unbiased exponent of a cluster's largest dev2 (subnormal or zero: -1022)
__device__ __forceinline__ int sil_exp(unsigned long long bits) {
  const int e = int((bits >> 52) & 0x7ffull);
  return e ? e - 1023 : -1022;
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_sil_wsum(const double* dev2, const int32_t* labels, int64_t n, int k,
                                                     const unsigned long long* wmax, unsigned long long* wsum) {
  extern __shared__ unsigned long long lw[];
  if (LDS) {
    for (int c = threadIdx.x; c < k; c += kBlock) lw[c] = 0ull;
    __syncthreads();
  }
  unsigned long long* dst = LDS ? lw : wsum;
  for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < n; p += int64_t(gridDim.x) * kBlock) {
    const int c = sil_label(labels[p], k);
    const long long q = __double2ll_rn(ldexp(dev2[p], kSilWBits - sil_exp(wmax[c])));
    if (q) atomicAdd(&dst[c], static_cast<unsigned long long>(q));
  }
  if (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kBlock)
      if (lw[c]) atomicAdd(&wsum[c], lw[c]);
  }
}

// wave per cluster
__global__ __launch_bounds__(kBlock) void k_sil_stats(const double* mean, const int64_t* sizes,
                                                      const unsigned long long* wmax,
                                                      const unsigned long long* wsum, int k, int d, int dp,
                                                      double* W, double* V, float* mu32, float* B) {
  const int lane = lane_id();
  for (int c = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; c < k; c += gridDim.x * (kBlock / kWave)) {
    const double* m = mean + int64_t(c) * d;
    double nrm = 0.0;
    for (int j = lane; j < dp; j += kWave) {
      const double v = j < d ? m[j] : 0.0;
      mu32[int64_t(c) * dp + j] = float(v);
      nrm = fma(v, v, nrm);
    }
    nrm = wave_sum(nrm);
    if (lane == 0) {
      const int64_t N = sizes[c];
      const double w = ldexp(double(static_cast<long long>(wsum[c])), sil_exp(wmax[c]) - kSilWBits);
      const double v = N > 0 ? w / double(N) : 0.0;
      W[c] = w;
      V[c] = v;
      B[c] = N > 0 ? float(nrm + v) : INFINITY;
    }
  }
}

void launch_sil_stats(const double* dev2, const int32_t* labels, int64_t n, int k, int d, int dp,
                      const double* mean, const int64_t* sizes, unsigned long long* wmax,
                      unsigned long long* wsum, double* W, double* V, float* mu32, float* B, hipStream_t s) {
  if (n <= 0 || n > kSilMaxRows) throw std::invalid_argument("launch_sil_stats: rows out of range");
  TWTML_HIP_CHECK(hipMemsetAsync(wmax, 0, sizeof(unsigned long long) * size_t(k), s));
  TWTML_HIP_CHECK(hipMemsetAsync(wsum, 0, sizeof(unsigned long long) * size_t(k), s));
  int grid = int((n + 4 * kBlock - 1) / (4 * kBlock));
  if (grid > 2048) grid = 2048;
  if (k <= 4 * kSilLdsBins) {
    const size_t lds = sizeof(unsigned long long) * size_t(k);
    TWTML_LAUNCH(k_sil_wmax<true>, dim3(grid), dim3(kBlock), lds, s, dev2, labels, n, k, wmax);
    TWTML_LAUNCH(k_sil_wsum<true>, dim3(grid), dim3(kBlock), lds, s, dev2, labels, n, k, wmax, wsum);
  } else {
    TWTML_LAUNCH(k_sil_wmax<false>, dim3(grid), dim3(kBlock), 0, s, dev2, labels, n, k, wmax);
    TWTML_LAUNCH(k_sil_wsum<false>, dim3(grid), dim3(kBlock), 0, s, dev2, labels, n, k, wmax, wsum);
  }
  int gs = (k + kBlock / kWave - 1) / (kBlock / kWave);
  if (gs > 4096) gs = 4096;
  TWTML_LAUNCH(k_sil_stats, dim3(gs), dim3(kBlock), 0, s, mean, sizes, wmax, wsum, k, d, dp, W, V, mu32, B);
}

// ---------------------------------------------------------------------------
// The neighbour pass.
// ---------------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;

// a lane's three smallest scores, ascending, with their clusters (-1: none;
// +inf, an empty or padded cluster, never enters)
struct SilTop3 {
  float v0 = INFINITY, v1 = INFINITY, v2 = INFINITY;
  int i0 = -1, i1 = -1, i2 = -1;
  __device__ __forceinline__ void add(float v, int c) {
    if (v < v2) {
      if (v < v1) {
        v2 = v1; i2 = i1;
        if (v < v0) { v1 = v0; i1 = i0; v0 = v; i0 = c; }
        else { v1 = v; i1 = c; }
      } else {
        v2 = v; i2 = c;
      }
    }
  }
  // the which-th (0, 1) best cluster that is not `own`
  __device__ __forceinline__ int other(int own, int which) const {
    const int c0 = i0 != own ? i0 : i1;
    const int c1 = (i0 != own && i1 != own) ? i1 : i2;
    return which == 0 ? c0 : c1;
  }
};

struct SilArgs {
  const float* X;
  const double* f64;
  const int32_t* labels;
  const double* dev2;
  const double* mean;
  const double* V;
  const double* W;
  const int64_t* sizes;
  int64_t n;
  int k, d, dp;
  int64_t* words;
  int32_t* neighbor;
  double *a, *b, *s;
};

// D(x_p, c) in fp64: k_km_cost's term, the columns in column order
__device__ __forceinline__ double sil_mean_dist(const SilArgs& g, int64_t p, int c) {
  const float* x = g.X + p * g.dp;
  const double* m = g.mean + int64_t(c) * g.d;
  double s = 0.0;
  for (int j = 0; j < g.d; ++j) {
    const double t = fma(double(x[j]), g.f64[j], -m[j]);
    s = fma(t, t, s);
  }
  return s + g.V[c];
}

// Every lane of the wave calls this (ballots); `valid` lanes own row p with
// the candidates (c0, D0), (c1, D1), c0 < 0: none.  lw: the workgroup's LDS
// words (n[k] | s_fix[k] | n_single) or nullptr.
__device__ __forceinline__ void sil_row(const SilArgs& g, bool valid, int64_t p, int own, int c0, double D0,
                                        int c1, double D1, unsigned long long* lw) {
  bool single = false;
  if (valid) {
    double b = 0.0, a = 0.0, sv = 0.0;
    int nb = -1;
    if (c0 >= 0) {
      b = D0; nb = c0;
      if (c1 >= 0 && (D1 < b || (D1 == b && c1 < nb))) { b = D1; nb = c1; }
    }
    const int64_t N = g.sizes[own];
    single = N == 1;
    if (nb >= 0 && !single) {
      a = (double(N) * g.dev2[p] + g.W[own]) / double(N - 1);
      if (a < b) sv = 1.0 - a / b;
      else if (a > b) sv = b / a - 1.0;
    }
    if (g.neighbor) {
      g.neighbor[p] = nb;
      g.a[p] = a;
      g.b[p] = b;
      g.s[p] = sv;
    }
    const long long fix = __double2ll_rn(sv * double(1ll << kSilFixBits));
    auto* dst = lw ? lw : reinterpret_cast<unsigned long long*>(g.words);
    atomicAdd(&dst[own], 1ull);
    if (fix) atomicAdd(&dst[g.k + own], static_cast<unsigned long long>(fix));
  }
  const uint64_t m = __ballot(single);
  if (m && lane_id() == 0) {
    auto* dst = lw ? lw : reinterpret_cast<unsigned long long*>(g.words);
    atomicAdd(&dst[2 * g.k], static_cast<unsigned long long>(__popcll(m)));
  }
}

__device__ __forceinline__ void sil_flush(const SilArgs& g, unsigned long long* lw) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * g.k + 1; i += kBlock)
    if (lw[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&g.words[i]), lw[i]);
}

// block = 4 waves = 128 points; the 32-cluster tile of mu32 is staged in LDS
// (rows padded to DP + 1 floats: conflict-free column reads).  A operand =
// clusters (lane: row l & 31, k = 2 s + (l >> 5)), B operand = points^T kept
// in VGPRs for the sweep.  D(32x32): lane l holds point l & 31 and clusters
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15.
template <int DP>
__global__ __launch_bounds__(kBlock) void k_sil_neighbor_mfma(SilArgs g, const float* fac, const float* mu32,
                                                              const float* B, int lds_words) {
  constexpr int KS = DP / 2;
  constexpr int LD = DP + 1;
  __shared__ float ct[32 * LD];
  __shared__ float cb[32];
  extern __shared__ unsigned long long lw_[];
  unsigned long long* lw = lds_words ? lw_ : nullptr;
  for (int i = threadIdx.x; i < lds_words; i += kBlock) lw_[i] = 0ull;
  const int lane = lane_id(), w = threadIdx.x / kWave;
  const int64_t p = int64_t(blockIdx.x) * 128 + w * 32 + (lane & 31);
  const int half = lane >> 5;
  const bool in = p < g.n;
  float xb[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) xb[s] = in ? g.X[p * DP + 2 * s + half] * fac[2 * s + half] : 0.f;
  SilTop3 t;
  for (int c0 = 0; c0 < g.k; c0 += 32) {
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * DP; i += kBlock) {
      const int r = i / DP, col = i % DP;
      ct[r * LD + col] = (c0 + r < g.k) ? mu32[int64_t(c0 + r) * DP + col] : 0.f;
    }
    if (threadIdx.x < 32) cb[threadIdx.x] = (c0 + int(threadIdx.x) < g.k) ? B[c0 + threadIdx.x] : INFINITY;
    __syncthreads();
    f32x16 acc = {};
    const float* crow = ct + (lane & 31) * LD + half;
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(crow[2 * s], xb[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cl = (r & 3) + 8 * (r >> 2) + 4 * half;
      t.add(fmaf(-2.f, acc[r], cb[cl]), c0 + cl);
    }
  }
  // both halves of a point's lane pair take the other's three: the pair then
  // holds the same top three, and half h measures candidate h
  const float o0 = __shfl_xor(t.v0, 32, kWave), o1 = __shfl_xor(t.v1, 32, kWave), o2 = __shfl_xor(t.v2, 32, kWave);
  const int j0 = __shfl_xor(t.i0, 32, kWave), j1 = __shfl_xor(t.i1, 32, kWave), j2 = __shfl_xor(t.i2, 32, kWave);
  t.add(o0, j0);
  t.add(o1, j1);
  t.add(o2, j2);
  const int own = in ? sil_label(g.labels[p], g.k) : 0;
  const int mine = in ? t.other(own, half) : -1;
  const double Dm = mine >= 0 ? sil_mean_dist(g, p, mine) : 0.0;
  const int c1 = __shfl_xor(mine, 32, kWave);
  const double D1 = __shfl_xor(Dm, 32, kWave);
  sil_row(g, in && half == 0, p, own, mine, Dm, c1, D1, lw);
  if (lw) sil_flush(g, lw);
}

// any width: one thread per point, scalar fp32 scores
__global__ __launch_bounds__(kBlock) void k_sil_neighbor_scalar(SilArgs g, const float* fac, const float* mu32,
                                                                const float* B, int lds_words) {
  extern __shared__ unsigned long long lw_[];
  unsigned long long* lw = lds_words ? lw_ : nullptr;
  for (int i = threadIdx.x; i < lds_words; i += kBlock) lw_[i] = 0ull;
  __syncthreads();
  const int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const bool in = p < g.n;
  SilTop3 t;
  if (in) {
    const float* x = g.X + p * g.dp;
    for (int c = 0; c < g.k; ++c) {
      const float* m = mu32 + int64_t(c) * g.dp;
      float dot = 0.f;
      for (int j = 0; j < g.dp; ++j) dot += m[j] * (x[j] * fac[j]);
      t.add(B[c] - 2.f * dot, c);
    }
  }
  const int own = in ? sil_label(g.labels[p], g.k) : 0;
  const int c0 = in ? t.other(own, 0) : -1, c1 = in ? t.other(own, 1) : -1;
  const double D0 = c0 >= 0 ? sil_mean_dist(g, p, c0) : 0.0;
  const double D1 = c1 >= 0 ? sil_mean_dist(g, p, c1) : 0.0;
  sil_row(g, in, p, own, c0, D0, c1, D1, lw);
  if (lw) sil_flush(g, lw);
}

void launch_sil_neighbor(const float* X, const float* f32, const double* f64, const int32_t* labels,
                         const double* dev2, int64_t n, int k, int d, int dp, const double* mean,
                         const float* mu32, const float* B, const double* V, const double* W,
                         const int64_t* sizes, bool mfma, int64_t* words, int32_t* neighbor, double* a,
                         double* b, double* sv, hipStream_t s) {
  if (n <= 0 || n > kSilMaxRows) throw std::invalid_argument("launch_sil_neighbor: rows out of range");
  const SilArgs g{X, f64, labels, dev2, mean, V, W, sizes, n, k, d, dp, words, neighbor, a, b, sv};
  const int lds_words = k <= kSilLdsBins ? 2 * k + 1 : 0;
  const size_t lds = sizeof(unsigned long long) * size_t(lds_words);
  bool done = false;
  if (mfma && dp >= 16 && dp <= 128 && k <= 4096) {
    const int grid = int((n + 127) / 128);
#define SIL_MFMA(DPV)                                                                                       \
  case DPV:                                                                                                 \
    TWTML_LAUNCH(k_sil_neighbor_mfma<DPV>, dim3(grid), dim3(kBlock), lds, s, g, f32, mu32, B, lds_words); \
    done = true;                                                                                            \
    break;
    switch (dp) { SIL_MFMA(16) SIL_MFMA(32) SIL_MFMA(64) SIL_MFMA(128) default: break; }
#undef SIL_MFMA
  }
  if (!done) {
    const int grid = int((n + kBlock - 1) / kBlock);
    TWTML_LAUNCH(k_sil_neighbor_scalar, dim3(grid), dim3(kBlock), lds, s, g, f32, mu32, B, lds_words);
  }
}

}  // namespace twtml
