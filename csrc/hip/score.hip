// Inference-only scoring of a raw batch with the fp64 master weights:
//
//     p(row) = sum over the row's bigram occurrences of w64[id]
//              + sum_k n_k * w64[F + k]
//
// with the hashed ids of the featurizer (featurize.hip: lower-casing, Java /
// murmur3 hashing, a 1-unit row is one term, a 0-unit row none) and the
// numeric features n_k formed in fp64 as MllibHelper.featurizeNumbers does
// (followers, favourites, friends * 1e-12, age in ms * 1e-14) -- not the
// fp32 values of the training path, and nothing rounded to whole retweets.
//
// The kernels walk the text exactly as the two featurizers do and gather
// weights where those write ids, so there is no entry-sized buffer at all:
//   k_score_narrow  fast chunks (16 Latin-1 rows of <= 4 * kFastMaxQ
//                   bigrams): text in VGPRs, contiguous quarters per lane
//                   (narrow_text.h);
//   k_score         every other chunk: 16 rows staged in LDS (text_stage.h);
//                   rows too long to stage read global memory.
// Sum order: in both kernels the row's 4 lanes take contiguous quarters of
// its bigrams (ceil(n / 4) each, the last ones fewer), each adds its entries
// in ascending order into an fp64 partial, the partials are added as
// (l0 + l1) + (l2 + l3) with quad DPP moves, then lane 0 adds the four numeric
// products in column order.  It is a function of the row alone -- not of the
// rows it shares a chunk with, hence not of the filter, the batch or the
// kernel either (k_featurize deals a slow chunk's entries round-robin; with
// that order here a narrow row in the chunk that straddles the narrow / wide
// boundary would sum differently than in a fast chunk).  No atomics, no
// cross-wave traffic: the same bits on every run.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "narrow_text.h"
#include "text_stage.h"

namespace twtml {

namespace {

// fp64 through a quad permute (two 32-bit DPP moves)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = uint32_t(__builtin_amdgcn_mov_dpp(int(uint32_t(u)), CTRL, 0xf, 0xf, true));
  const uint32_t hi = uint32_t(__builtin_amdgcn_mov_dpp(int(uint32_t(u >> 32)), CTRL, 0xf, 0xf, true));
  return __builtin_bit_cast(double, (uint64_t(hi) << 32) | lo);
}

// (l0 + l1) + (l2 + l3) over the 4 lanes of a row; every lane of the quad
// must be active.  fp64 addition commutes, so all four lanes hold the same bits.
__device__ __forceinline__ double quad_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  return v;
}

// What a score is of the margin (launch_score's link).
struct ScoreLink {
  int32_t link;
  double logit_thr;
};

// Lane t == 0 of a row: numeric part (fp64, MllibHelper.scala:58-71), the
// link, and the store at the row's kept index.
__device__ __forceinline__ void score_store(const DevRawBatch& b, const FeaturizeParams& fp, const double* w64,
                                            double text, int64_t row, int32_t kidx, double* pred,
                                            int64_t* rows, const ScoreLink& lk) {
  const double* wn = w64 + fp.num_text_features;
  double p = text;
  p += (double(raw_scalar(b, 1, row)) * 1e-12) * wn[0];
  p += (double(raw_scalar(b, 2, row)) * 1e-12) * wn[1];
  p += (double(raw_scalar(b, 3, row)) * 1e-12) * wn[2];
  p += (double(fp.now_ms - raw_scalar(b, 4, row)) * 1e-14) * wn[3];
  if (lk.link == kLinkProbability) p = 1.0 / (1.0 + exp(-p));   // exp overflows to +inf: exactly 0
  else if (lk.link == kLinkClass) p = p > lk.logit_thr ? 1.0 : 0.0;
  pred[kidx] = p;
  if (rows) rows[kidx] = row;
}

// (A variant with w64[0, 8161) -- every id of a Java-hashed Latin-1 bigram,
// NarrowHash::direct -- staged in 64 KB of LDS per workgroup was measured
// and dropped: 0.524 ms against 0.501 ms for 1M wide-profile tweets; the
// gathers of the hot ids hit L2 anyway and the table costs occupancy,
// profiles/README.md "Scoring".)
__global__ __launch_bounds__(kBlock) void k_score_narrow(DevRawBatch b, DevPrepared p, FeaturizeParams fp,
                                                         const double* w64, double* pred, int64_t* rows,
                                                         int64_t cmax, ScoreLink lk) {
  const int64_t n_kept = p.counters[0];
  const int t = lane_id() % kLanesPerRow;
  const int64_t wave = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = int64_t(gridDim.x) * kBlock / kWave;
  const NarrowHash nh(fp);
  const int64_t nch = (n_kept + kRowsPerChunk - 1) / kRowsPerChunk;
  for (int64_t c = wave; c < nch && c < cmax; c += nwaves) {
    if (!p.cfast[c]) continue;
    const int32_t L8 = p.clen8[c];
    NarrowLane L;
    uint32_t a[kFastAl];
    narrow_lane_load(b, p, c, n_kept, L, a);
    double acc = 0.0;
#pragma unroll
    for (int g = 0; g < kFastMaxQ / kGroup; ++g) {
      if (g >= L8) break;                               // wave-uniform
      double wv[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const int e = g * kGroup + k;
        const int64_t id = narrow_id(L, a, e, nh);
        wv[k] = e < L.my ? w64[id] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k)
        if (g * kGroup + k < L.my) acc += wv[k];
    }
    acc = quad_sum_f64(acc);
    if (t == 0 && L.valid) score_store(b, fp, w64, acc, L.row, L.kidx, pred, rows, lk);
  }
}

__global__ __launch_bounds__(kBlock) void k_score(DevRawBatch b, DevPrepared p, FeaturizeParams fp,
                                                  const uint8_t* lpage, const uint16_t* lblocks,
                                                  const double* w64, double* pred, int64_t* rows, int64_t cmax,
                                                  ScoreLink lk) {
  __shared__ uint32_t stage[kBlock / kWave][kRowsPerChunk * kStageStride];
  __shared__ __attribute__((aligned(16))) uint8_t lpage_s[256];
  __shared__ __attribute__((aligned(16))) uint16_t lblk_s[kLowerLdsBlocks * 256];
  stage_lower_tables(lpage_s, lblk_s, lpage, lblocks, threadIdx.x, kBlock);
  __syncthreads();
  const LowerLds lt{lpage_s, lblk_s, lblocks};
  const int64_t n_kept = p.counters[0];
  const int lane = lane_id();
  const int r = lane / kLanesPerRow, t = lane % kLanesPerRow;
  uint32_t* st = stage[threadIdx.x / kWave];
  const int64_t wave = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = int64_t(gridDim.x) * kBlock / kWave;
  const int64_t F = fp.num_text_features;
  const bool f32 = F <= 0xffffffffLL;
  const FastMod32 fm(f32 ? uint32_t(F) : 1u);
  const int64_t nch = (n_kept + kRowsPerChunk - 1) / kRowsPerChunk;
  for (int64_t c = wave; c < nch && c < cmax; c += nwaves) {
    if (p.cfast[c]) continue;            // k_score_narrow's chunk
    const int32_t L8 = p.clen8[c];
    // row metadata (lane l resolves row l & 15), then the 16 rows into LDS
    const int64_t mpos = c * kRowsPerChunk + (lane & 15);
    const bool mvalid = mpos < n_kept;
    const int32_t mkidx = mvalid ? p.sorted[mpos] : -1;
    const StageMeta meta = stage_meta(b, mvalid, mvalid ? p.kept[mkidx] : 0);
    stage_rows(b, meta, st, lane);
    const int64_t pos = c * kRowsPerChunk + r;
    const bool valid = pos < n_kept;
    const int32_t kidx = __shfl(mkidx, r, kWave);
    const int64_t row = __shfl(meta.row, r, kWave);
    const StagedRow sr = staged_row(meta, st, r);
    const int64_t len = valid ? sr.rt.len : 0;
    const int64_t nz = len >= 2 ? len - 1 : len;
    // The row's 4 lanes take the same contiguous quarters as k_score_narrow's
    // (narrow_lane_text), each in ascending entry order: a row sums in the
    // same order whichever kernel its chunk falls to.  A lane reads each of
    // its units once (an entry's second unit is the next entry's first).
    const int32_t q = int32_t((nz + kLanesPerRow - 1) / kLanesPerRow);
    const int64_t e0 = int64_t(t) * q;
    const int32_t my = nz - e0 < 0 ? 0 : (nz - e0 < q ? int32_t(nz - e0) : q);
    const int32_t total = L8 * kGroup;   // wave-uniform bound of `my`
    double acc = 0.0;
    uint32_t u0 = my > 0 ? sr.unit(b, e0, lt) : 0u;
    for (int32_t g0 = 0; g0 < total; g0 += kGroup) {
      double wv[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const int32_t e = g0 + k;
        wv[k] = 0.0;
        if (e < my) {
          int64_t h;
          if (len >= 2) {
            const uint32_t u1 = sr.unit(b, e0 + e + 1, lt);
            h = fp.hash_kind == 0 ? int64_t(31u * u0 + u1) : int64_t(murmur_term(u0, u1, 2));
            u0 = u1;
          } else {
            h = fp.hash_kind == 0 ? int64_t(u0) : int64_t(murmur_term(u0, 0, 1));
          }
          wv[k] = w64[term_mod(h, F, fm, f32)];
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k)
        if (g0 + k < my) acc += wv[k];
    }
    __builtin_amdgcn_wave_barrier();   // LDS reads of this chunk precede the next staging
    acc = quad_sum_f64(acc);
    if (t == 0 && valid) score_store(b, fp, w64, acc, row, kidx, pred, rows, lk);
  }
}

// counters and the length histogram of a scoring-only DevPrepared (the part
// of k_prep_init such a buffer has arrays for)
__global__ __launch_bounds__(1024) void k_score_init(int64_t* counters, int64_t* hist) {
  const int i = int(blockIdx.x) * 1024 + threadIdx.x;
  if (i < 8) counters[i] = 0;
  if (i < kLenBuckets + 1) hist[i] = 0;
}

}  // namespace

void launch_score_init(const DevPrepared& p, hipStream_t s) {
  TWTML_LAUNCH(k_score_init, dim3(ceil_div(kLenBuckets + 1, 1024)), dim3(1024), 0, s, p.counters, p.hist);
}

void launch_score(const DevRawBatch& b, const DevPrepared& p, const FeaturizeParams& fp, const uint8_t* lpage,
                  const uint16_t* lblocks, const double* w64, double* pred, int64_t* rows, hipStream_t s,
                  int link, double logit_thr) {
  const int64_t cmax = (b.n + kRowsPerChunk - 1) / kRowsPerChunk;
  if (cmax == 0) return;
  int grid = ceil_div(cmax, kBlock / kWave);
  if (grid > 2048) grid = 2048;
  const ScoreLink lk{link, logit_thr};
  TWTML_LAUNCH(k_score_narrow, dim3(grid), dim3(kBlock), 0, s, b, p, fp, w64, pred, rows, cmax, lk);
  TWTML_LAUNCH(k_score, dim3(grid), dim3(kBlock), 0, s, b, p, fp, lpage, lblocks, w64, pred, rows, cmax, lk);
}

}  // namespace twtml
