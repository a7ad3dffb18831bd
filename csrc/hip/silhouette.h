// Launchers of the silhouette kernels (silhouette.hip): the batch's cluster
// statistics and the neighbour pass of KMEngine::silhouette.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace twtml {

// Result words of one batch: n[k] | s_fix[k] | n_single | n_undefined |
// non-empty clusters | rows scored.
constexpr int kSilTail = 4;
inline size_t sil_words(int k) { return 2 * size_t(k) + kSilTail; }
// W's fixed point: rint(dev2 2^(kSilWBits - e)), e the exponent of the
// cluster's largest dev2, summed in int64: |q| <= 2^(kSilWBits + 1), so a
// batch of up to kSilMaxRows rows cannot overflow.
constexpr int kSilWBits = 40;
constexpr int64_t kSilMaxRows = int64_t(1) << 22;
constexpr int kSilFixBits = 36;   // s_fix = sum rint(s 2^36) (models/silhouette.py)

// mean[c][j] = counts[c] > 0 ? sums[c][j] / counts[c] : 0 (fp64, one division)
void launch_sil_means(const double* sums, const double* counts, int k, int d, double* mean, hipStream_t s);
// W[c] = sum of dev2 over the rows labelled c, bit-reproducible: per-cluster
// max of dev2 (integer atomic max on the bit pattern), then the int64 sum of
// rint(dev2 2^(40 - e)); wmax / wsum: [k] scratch, zeroed here.  Then per
// cluster V = W / N, mu32 (fp32 means padded to dp), B = |mu|^2 + V in fp32
// (+inf for an empty cluster).
void launch_sil_stats(const double* dev2, const int32_t* labels, int64_t n, int k, int d, int dp,
                      const double* mean, const int64_t* sizes, unsigned long long* wmax,
                      unsigned long long* wsum, double* W, double* V, float* mu32, float* B, hipStream_t s);
// The neighbour pass: fp32 scores B - 2 x.mu on the matrix cores (mfma and
// 16 <= dp <= 128 and k <= 4096) or scalar, the two best other clusters
// re-measured in fp64, then a, b, s and the integer words.  a / b / sv /
// neighbor: per-row outputs or all nullptr.  words: zeroed by the caller.
void launch_sil_neighbor(const float* X, const float* f32, const double* f64, const int32_t* labels,
                         const double* dev2, int64_t n, int k, int d, int dp, const double* mean,
                         const float* mu32, const float* B, const double* V, const double* W,
                         const int64_t* sizes, bool mfma, int64_t* words, int32_t* neighbor, double* a,
                         double* b, double* sv, hipStream_t s);

}  // namespace twtml
