// Exact, deterministic per-cluster top-m selection over a device array of fp64
// values and their int32 labels (exemplars.hip): the contract of
// twitter_stream_ml_amd/models/exemplars.py.
//
//   values[0 .. cnt)   one per scored row, in scored order; cnt is read from a
//                      device word (counters[0]) and clamped to `cap`
//   labels[0 .. cnt)   the row's cluster, in [0, k)
//   rows               raw row id of scored row i, ascending (null: i)
//   sizes[k]           rows per cluster (NaN rows included), as the cost pass
//                      of score() leaves them
// Within a cluster: best value first (ascending; descending with `largest`),
// values compare as IEEE numbers (-0.0 == +0.0), equal values by ascending
// scored index (= ascending raw row id).  NaN values are never selected
// (counted in n_nan, a batch total).  Nothing is synchronised with the host.
//
// Result block `out` (int64 words): [kExNNan], [kExCnt] the clamped cnt, then k
// counts = min(m, rows of c that are not NaN), k*m words of value bits (the
// original bits; 0 in unused entries) and k*m raw row ids (-1 in unused
// entries), cluster-major, each cluster best first.  The same bits on every
// call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace twtml {

constexpr int kExMaxM = 64;                 // largest m
constexpr int64_t kExMaxCells = 1 << 18;    // largest k * m
constexpr int kExTile = 2048;               // scored rows per workgroup of the tile pass
constexpr int kExChunk = 4096;              // candidates a merge workgroup sorts at once
constexpr int kExHead = 4;
constexpr int kExNNan = 0, kExCnt = 1;
constexpr size_t ex_out_words(int64_t k, int m) { return size_t(kExHead) + size_t(k) + 2 * size_t(k) * size_t(m); }

// Device scratch of one selection; carve() lays it out in a buffer of
// ex_scratch_words(cap, kcap) int64 words: good for every cap' <= cap and
// every (k, m) with k <= kcap and ex_out_words(k, m) <= ex_out_words(kcap, m0)
// for the m0 it was sized with.
struct ExScratch {
  uint32_t* zero = nullptr;     // [2] NaN count | [kcap] per-cluster candidate cursors; zeroed per call
  uint32_t* base = nullptr;     // [kcap + 1] exclusive scan of the sizes
  uint64_t* ckey = nullptr;     // [cap] candidates' value keys, cluster c's from base[c]
  uint32_t* cidx = nullptr;     // [cap] candidates' scored indices
  int64_t* out = nullptr;       // [out_words] result block
  size_t zero_bytes = 0;
  int64_t cap = 0, kcap = 0;
  size_t out_words = 0;
};
size_t ex_scratch_words(int64_t cap, int64_t kcap, size_t out_words);
ExScratch ex_scratch_carve(int64_t* base, int64_t cap, int64_t kcap, size_t out_words);

// Rows per cluster of labels[0 .. cnt) (labels outside [0, k) are not counted),
// for callers that have no cost pass before them.
void launch_cluster_sizes(const int32_t* labels, const int64_t* counters, int64_t cap, int k, int64_t* sizes,
                          hipStream_t s);

// Select on `s`: the scan of the sizes, the tile pass, the merge pass.
// 1 <= m <= kExMaxM, k * m <= kExMaxCells, cap < 2^31 and within the scratch.
void launch_cluster_select(const double* values, const int32_t* labels, const int64_t* rows, const int64_t* counters,
                           int64_t cap, int k, int m, bool largest, const int64_t* sizes, const ExScratch& sc,
                           hipStream_t s);

}  // namespace twtml
