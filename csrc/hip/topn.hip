// Exact top-N selection over a device array of fp64 values (topn.h), behind
// the scoring passes of both engines: the N best rows leave the device, not
// the predictions.
//
// Composite key of scored row k (never NaN): the order-preserving unsigned
// image of the value (sign flip; -0.0 canonicalised to +0.0; inverted for
// "smallest"), extended with the inverted scored index ~k.  Composite keys are
// unique and "larger" means "earlier in the result", so ties need no separate
// handling: the N best rows are the N largest composite keys.
//
//   k_top_hist     pass p = 0 .. 8, most significant digit first: the digit
//                  histogram of the keys that share the prefix chosen so far.
//                  Workgroup-private uint32 histogram in LDS (non-returning
//                  adds; a wave whose lanes all hold one digit adds once),
//                  flushed for its non-zero bins with integer global atomics
//                  -- exact in any order.  Every workgroup of pass p first
//                  resolves pass p - 1's global histogram (top_resolve): the
//                  bin that holds the n-th key extends the prefix.  Nothing
//                  left to decide (the bin holds exactly what is still
//                  needed, or cnt - n_nan <= n): the pass returns at once.
//   k_top_collect  resolves the last histogram, then gathers the keys at or
//                  beyond the threshold.  There are exactly n_top of them, so
//                  their arrival order comes from a returning atomic cursor
//                  (one add per wave).
//   k_top_sort     one workgroup: bitonic sort of the gathered keys in LDS
//                  (4096 x 12 B), which fixes the output order, then the
//                  original value bits, raw row ids and payloads.
// No float atomics, no scratch memory, no host round trip.
#include <hip/hip_runtime.h>

#include "common.h"
#include "topn.h"

namespace twtml {

namespace {

constexpr int kStateWords = 8;
constexpr int kStHi = 0, kStLo = 1, kStNeed = 2, kStDone = 3, kStNTop = 4, kStNNan = 5, kStCnt = 6;
constexpr int kBinsPerThread = kTopBins / kBlock;
constexpr int kSortBlock = 1024;
static_assert(kTopBins % kBlock == 0, "top_resolve deals the bins evenly");

// digit p of the composite key: its word (value key for p < 6, else the
// index word), its shift and its width
__device__ __forceinline__ int top_shift(int p) { return p < 5 ? 53 - 11 * p : (p == 5 ? 0 : (p == 6 ? 21 : (p == 7 ? 10 : 0))); }
__device__ __forceinline__ int top_width(int p) { return p == 5 ? 9 : (p == 8 ? 10 : 11); }

__device__ __forceinline__ uint64_t top_key(double v, int largest) {
  uint64_t u = __builtin_bit_cast(uint64_t, v);
  if ((u << 1) == 0) u = 0;   // -0.0 == +0.0
  const uint64_t k = (u >> 63) ? ~u : (u | (uint64_t(1) << 63));
  return largest ? k : ~k;
}

__device__ __forceinline__ uint32_t top_cnt(const int64_t* counters, int64_t cap) {
  const int64_t c = counters[0];
  return uint32_t(c < 0 ? 0 : (c > cap ? cap : c));
}

struct TopSel {
  uint64_t hi = 0;     // value-key part of the prefix (threshold once done; lower digits zero)
  uint32_t lo = 0;     // index part
  uint32_t need = 0;   // entries still to take inside the prefix
  uint32_t done = 0;
  uint32_t n_top = 0, n_nan = 0;
};

// The state after pass q from its global histogram and the state before it
// (st_in; none for q = 0).  Bins are walked from the top: the bin where the
// running count reaches `need` extends the prefix, the bins above it are
// taken whole.  Every workgroup computes the same; workgroup 0 records it in
// st_out for the next launch.  sh: 8 words of LDS.  Whole workgroup.
__device__ __forceinline__ TopSel top_resolve(int q, const uint32_t* hist, const uint64_t* st_in, uint64_t* st_out,
                                              uint32_t cnt, uint32_t n, uint32_t* sh) {
  TopSel r;
  if (q > 0) {
    r.hi = st_in[kStHi];
    r.lo = uint32_t(st_in[kStLo]);
    r.need = uint32_t(st_in[kStNeed]);
    r.done = uint32_t(st_in[kStDone]);
    r.n_top = uint32_t(st_in[kStNTop]);
    r.n_nan = uint32_t(st_in[kStNNan]);
  }
  if (!r.done) {   // uniform over the workgroup
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    if (t < 8) sh[t] = 0;
    // descending bins: position i = kTopBins - 1 - bin; thread t owns kBinsPerThread of them
    uint32_t h[kBinsPerThread], sum = 0;
#pragma unroll
    for (int j = 0; j < kBinsPerThread; ++j) {
      h[j] = hist[kTopBins - 1 - (kBinsPerThread * t + j)];
      sum += h[j];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t v = uint32_t(__shfl_up(int(inc), off, kWave));
      if (lane >= off) inc += v;
    }
    __syncthreads();
    if (lane == kWave - 1) sh[wave] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      if (w < wave) base += sh[w];
      total += sh[w];
    }
    if (q == 0) {
      r.n_nan = cnt - total;
      r.n_top = n < total ? n : total;
      r.need = r.n_top;
      if (total <= n) r.done = 1;   // everything is taken: threshold 0
    }
    if (!r.done) {
      uint32_t e = base + inc - sum;
#pragma unroll
      for (int j = 0; j < kBinsPerThread; ++j) {
        if (e < r.need && r.need <= e + h[j]) {   // exactly one bin of one thread
          sh[4] = uint32_t(kTopBins - 1 - (kBinsPerThread * t + j));
          sh[5] = e;
          sh[6] = h[j];
        }
        e += h[j];
      }
      __syncthreads();
      const uint32_t bin = sh[4], before = sh[5], c = sh[6];
      if (q < 6) r.hi |= uint64_t(bin) << top_shift(q);
      else r.lo |= bin << top_shift(q);
      r.need -= before;
      r.done = c == r.need ? 1 : 0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st_out[kStHi] = r.hi;
    st_out[kStLo] = r.lo;
    st_out[kStNeed] = r.need;
    st_out[kStDone] = r.done;
    st_out[kStNTop] = r.n_top;
    st_out[kStNNan] = r.n_nan;
    st_out[kStCnt] = cnt;
  }
  return r;
}

__global__ __launch_bounds__(kBlock) void k_top_hist(const double* values, const int64_t* counters, int64_t cap,
                                                     uint32_t n, int largest, int p, uint32_t* hist_all,
                                                     uint64_t* state_all) {
  __shared__ uint32_t h[kTopBins];
  __shared__ uint32_t sh[8];
  for (int i = threadIdx.x; i < kTopBins; i += kBlock) h[i] = 0;
  const uint32_t cnt = top_cnt(counters, cap);
  TopSel r;
  if (p > 0) {
    r = top_resolve(p - 1, hist_all + size_t(p - 1) * kTopBins, state_all + size_t(p - 1) * kStateWords,
                    state_all + size_t(p) * kStateWords, cnt, n, sh);
    if (r.done) return;
  }
  __syncthreads();
  // keys of this pass: the bits above digit p equal the prefix
  const int shift = top_shift(p), width = top_width(p);
  const uint32_t dmask = (1u << width) - 1u;
  const uint64_t mhi = p >= 6 ? ~uint64_t(0) : (shift + width >= 64 ? 0 : ~uint64_t(0) << (shift + width));
  const uint32_t mlo = p < 6 ? 0u : (shift + width >= 32 ? 0u : ~0u << (shift + width));
  const int lane = lane_id();
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t k0 = blockIdx.x * kBlock + (threadIdx.x - lane); k0 < cnt; k0 += stride) {
    const uint32_t k = k0 + lane;
    bool ok = k < cnt;
    uint32_t d = 0;
    if (ok) {
      const double v = values[k];
      const uint64_t hi = top_key(v, largest);
      const uint32_t lo = ~k;
      ok = v == v && ((hi ^ r.hi) & mhi) == 0 && ((lo ^ r.lo) & mlo) == 0;
      d = p < 6 ? uint32_t(hi >> shift) & dmask : (lo >> shift) & dmask;
    }
    const uint64_t m = __ballot(ok);
    if (m == 0) continue;
    // equal digits of a wave are combined before the LDS add when the whole
    // wave agrees (all-equal values: every lane hits one bin)
    const int first = __ffsll((unsigned long long)m) - 1;
    const uint32_t d0 = uint32_t(__shfl(int(d), first, kWave));
    if (__ballot(ok && d == d0) == m) {
      if (lane == first) atomicAdd(&h[d0], uint32_t(__popcll(m)));
    } else if (ok) {
      atomicAdd(&h[d], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = hist_all + size_t(p) * kTopBins;
  for (int i = threadIdx.x; i < kTopBins; i += kBlock) {
    const uint32_t v = h[i];
    if (v) atomicAdd(&out[i], v);
  }
}

__global__ __launch_bounds__(kBlock) void k_top_collect(const double* values, const int64_t* counters, int64_t cap,
                                                        uint32_t n, int largest, uint32_t* hist_all,
                                                        uint64_t* state_all, uint32_t* cursor, uint64_t* ckey,
                                                        uint32_t* cidx) {
  __shared__ uint32_t sh[8];
  const uint32_t cnt = top_cnt(counters, cap);
  const TopSel r = top_resolve(kTopPasses - 1, hist_all + size_t(kTopPasses - 1) * kTopBins,
                               state_all + size_t(kTopPasses - 1) * kStateWords,
                               state_all + size_t(kTopPasses) * kStateWords, cnt, n, sh);
  if (r.n_top == 0) return;
  const int lane = lane_id();
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t k0 = blockIdx.x * kBlock + (threadIdx.x - lane); k0 < cnt; k0 += stride) {
    const uint32_t k = k0 + lane;
    bool ok = k < cnt;
    uint64_t hi = 0;
    if (ok) {
      const double v = values[k];
      hi = top_key(v, largest);
      const uint32_t lo = ~k;
      ok = v == v && (hi > r.hi || (hi == r.hi && lo >= r.lo));
    }
    const uint64_t m = __ballot(ok);
    if (m == 0) continue;
    const int first = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(cursor, uint32_t(__popcll(m)));
    base = uint32_t(__shfl(int(base), first, kWave));
    const uint32_t pos = base + uint32_t(__popcll(m & ((uint64_t(1) << lane) - 1u)));
    if (ok && pos < r.n_top && pos < uint32_t(kTopNMax)) {
      ckey[pos] = hi;
      cidx[pos] = k;
    }
  }
}

__global__ __launch_bounds__(kSortBlock) void k_top_sort(const double* values, const int64_t* rows,
                                                         const int32_t* payload, const uint64_t* st,
                                                         const uint64_t* ckey, const uint32_t* cidx, uint32_t n,
                                                         int64_t* out) {
  __shared__ uint64_t sk[kTopNMax];
  __shared__ uint32_t si[kTopNMax];
  const uint32_t cnt = uint32_t(st[kStCnt]);
  uint32_t n_top = uint32_t(st[kStNTop]);
  if (n_top > n) n_top = n;
  uint32_t m = 2;
  while (m < n_top) m <<= 1;   // n_top <= n <= kTopNMax
  // pads (key 0, index all ones) are below every entry
  for (uint32_t i = threadIdx.x; i < m; i += kSortBlock) {
    sk[i] = i < n_top ? ckey[i] : 0;
    si[i] = i < n_top ? cidx[i] : ~0u;
  }
  __syncthreads();
  // bitonic network, best first: larger key, then smaller index
  for (uint32_t k = 2; k <= m; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < m; i += kSortBlock) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t ka = sk[i], kb = sk[l];
          const uint32_t ia = si[i], ib = si[l];
          const bool a_first = ka > kb || (ka == kb && ia < ib);
          if (((i & k) == 0) != a_first) {
            sk[i] = kb;
            sk[l] = ka;
            si[i] = ib;
            si[l] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < n; i += kSortBlock) {
    const uint32_t idx = i < n_top ? si[i] : ~0u;
    const bool ok = idx < cnt;
    out[kTopHead + i] = ok ? __builtin_bit_cast(int64_t, values[idx]) : 0;
    out[kTopHead + n + i] = ok ? (rows ? rows[idx] : int64_t(idx)) : 0;
    out[kTopHead + 2 * size_t(n) + i] = ok && payload ? int64_t(payload[idx]) : 0;
  }
  if (threadIdx.x == 0) {
    out[kTopNTop] = n_top;
    out[kTopNNan] = int64_t(st[kStNNan]);
    out[kTopCnt] = cnt;
    out[3] = 0;
  }
}

constexpr size_t kHistBytes = sizeof(uint32_t) * size_t(kTopPasses) * kTopBins;
constexpr size_t kStateBytes = sizeof(uint64_t) * size_t(kTopPasses + 1) * kStateWords;
constexpr size_t kCursorBytes = 8;
constexpr size_t kKeyBytes = sizeof(uint64_t) * size_t(kTopNMax);
constexpr size_t kIdxBytes = sizeof(uint32_t) * size_t(kTopNMax);
static_assert(kHistBytes % 8 == 0 && kIdxBytes % 8 == 0, "every part starts on an 8-byte boundary");

}  // namespace

size_t top_scratch_words() {
  return (kHistBytes + kStateBytes + kCursorBytes + kKeyBytes + kIdxBytes) / 8 + top_out_words(kTopNMax);
}

TopScratch top_scratch_carve(int64_t* base) {
  TopScratch sc;
  char* p = reinterpret_cast<char*>(base);
  sc.hist = reinterpret_cast<uint32_t*>(p);
  p += kHistBytes;
  sc.state = reinterpret_cast<uint64_t*>(p);
  p += kStateBytes;
  sc.cursor = reinterpret_cast<uint32_t*>(p);
  p += kCursorBytes;
  sc.zero_bytes = kHistBytes + kStateBytes + kCursorBytes;
  sc.ckey = reinterpret_cast<uint64_t*>(p);
  p += kKeyBytes;
  sc.cidx = reinterpret_cast<uint32_t*>(p);
  p += kIdxBytes;
  sc.out = reinterpret_cast<int64_t*>(p);
  return sc;
}

int top_grid(int64_t cap) {
  const int g = ceil_div(cap, kBlock);
  return g < 1 ? 1 : (g > kTopMaxGrid ? kTopMaxGrid : g);
}

void launch_top_select(const double* values, const int64_t* rows, const int32_t* payload, const int64_t* counters,
                       int64_t cap, int n, bool largest, const TopScratch& sc, hipStream_t s) {
  if (n < 1 || n > kTopNMax) throw std::invalid_argument("top-N: n must be in [1, 4096]");
  if (cap < 0 || cap >= (int64_t(1) << 31)) throw std::invalid_argument("top-N: capacity out of range");
  TWTML_HIP_CHECK(hipMemsetAsync(sc.hist, 0, sc.zero_bytes, s));
  const int grid = top_grid(cap);
  const int lg = largest ? 1 : 0;
  for (int p = 0; p < kTopPasses; ++p)
    TWTML_LAUNCH(k_top_hist, dim3(grid), dim3(kBlock), 0, s, values, counters, cap, uint32_t(n), lg, p, sc.hist,
                 sc.state);
  TWTML_LAUNCH(k_top_collect, dim3(grid), dim3(kBlock), 0, s, values, counters, cap, uint32_t(n), lg, sc.hist,
               sc.state, sc.cursor, sc.ckey, sc.cidx);
  TWTML_LAUNCH(k_top_sort, dim3(1), dim3(kSortBlock), 0, s, values, rows, payload,
               sc.state + size_t(kTopPasses) * kStateWords, sc.ckey, sc.cidx, uint32_t(n), sc.out);
}

}  // namespace twtml
