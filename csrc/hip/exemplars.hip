// Exact per-cluster top-m selection (exemplars.h), behind the scoring passes
// of the k-means engine: k x m rows leave the device, not the labels and the
// distances of every row.
//
// Composite key of scored row i (never NaN): (label, value key, i), ascending.
// The value key is the order-preserving unsigned image of the value (sign flip;
// -0.0 canonicalised to +0.0; inverted for "largest"), so a smaller key is a
// better value.  Composite keys are unique: the answer is fixed by the
// contract alone, whatever the order in which candidates are generated.
//
//   k_ex_scan    one workgroup: base = exclusive scan of the cluster sizes.
//   k_ex_tile    one workgroup per tile of kExTile consecutive scored rows:
//                NaNs dropped and counted (ballot, one integer add per wave),
//                bitonic sort of the tile in LDS by the composite key; a
//                sorted position whose rank inside its label run is < m is a
//                candidate and goes to cand[base[label] + cursor[label]++] --
//                one returning integer atomic per (tile, run), taken by the
//                run's head for all of the run's candidates.  A cluster's
//                candidates are a subset of its rows: the capacity is exact.
//   k_ex_merge   workgroups stride over the clusters.  A cluster's candidates
//                pass through LDS in chunks of kExChunk: sort, keep the best
//                m, refill with the next kExChunk - m.  Then the counts, the
//                original value bits and the raw row ids; empty clusters
//                write count 0 and the padding.
//
// LDS: the keys are kept as separate arrays of 8-byte (and 4-byte) words, not
// as 16-byte records, and a compare-exchange step deals pair t of the network
// to thread t.  For a distance j >= 32 the lanes of a half-wave read
// consecutive words (conflict-free); below that they read two runs of words
// 2j apart, at most two lanes per bank.  Tile pass 40 KB, merge pass 48 KB per
// workgroup: three of either fit a CU's 160 KB.
// No float atomics, no scratch memory, no host round trip.
#include <hip/hip_runtime.h>

#include "common.h"
#include "exemplars.h"

namespace twtml {

namespace {

constexpr int kExBlock = 1024;
constexpr int kExWaves = kExBlock / kWave;
constexpr int kExMergeGrid = 512;
constexpr uint32_t kNoLabel = ~0u;
static_assert(kExTile == 2 * kExBlock, "the tile pass deals one pair of the network to each thread");
static_assert(kExChunk % kExBlock == 0 && kExChunk >= 2 * kExMaxM, "a refill brings at least kExMaxM new candidates");
static_assert((kExTile & (kExTile - 1)) == 0 && (kExChunk & (kExChunk - 1)) == 0, "bitonic sizes");

// smaller = better; never 0 or all ones (those are images of NaNs)
__device__ __forceinline__ uint64_t ex_key(double v, int largest) {
  uint64_t u = __builtin_bit_cast(uint64_t, v);
  if ((u << 1) == 0) u = 0;   // -0.0 == +0.0
  const uint64_t k = (u >> 63) ? ~u : (u | (uint64_t(1) << 63));
  return largest ? ~k : k;
}

__device__ __forceinline__ uint32_t ex_cnt(const int64_t* counters, int64_t cap) {
  const int64_t c = counters[0];
  return uint32_t(c < 0 ? 0 : (c > cap ? cap : c));
}

__device__ __forceinline__ uint32_t ex_size(int64_t v) {
  return uint32_t(v < 0 ? 0 : (v > int64_t(0x7FFFFFFF) ? int64_t(0x7FFFFFFF) : v));
}

// pair t of a compare-exchange step at distance j: positions i and i | j
__device__ __forceinline__ uint32_t ex_pair_lo(uint32_t t, uint32_t j) { return ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); }

__global__ __launch_bounds__(kBlock) void k_ex_sizes(const int32_t* labels, const int64_t* counters, int64_t cap,
                                                     int k, int64_t* sizes) {
  const uint32_t cnt = ex_cnt(counters, cap);
  const int lane = lane_id();
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t i0 = blockIdx.x * kBlock + (threadIdx.x - lane); i0 < cnt; i0 += stride) {
    const uint32_t i = i0 + lane;
    uint32_t lab = kNoLabel;
    if (i < cnt) lab = uint32_t(labels[i]);
    const bool ok = lab < uint32_t(k);
    const uint64_t mk = __ballot(ok);
    if (mk == 0) continue;
    // a wave whose rows all carry one label adds once
    const int first = __ffsll((unsigned long long)mk) - 1;
    const uint32_t l0 = uint32_t(__shfl(int(lab), first, kWave));
    if (__ballot(ok && lab == l0) == mk) {
      if (lane == first) atomicAdd(reinterpret_cast<unsigned long long*>(&sizes[l0]), (unsigned long long)__popcll(mk));
    } else if (ok) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&sizes[lab]), 1ull);
    }
  }
}

// base[0 .. k] = exclusive scan of the clamped sizes; thread t owns the
// consecutive clusters [t per, (t + 1) per)
__global__ __launch_bounds__(kExBlock) void k_ex_scan(const int64_t* sizes, int k, uint32_t* base) {
  __shared__ uint32_t sh[kExWaves];
  const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
  const int per = (k + kExBlock - 1) / kExBlock;
  const int lo = t * per < k ? t * per : k, hi = lo + per < k ? lo + per : k;
  uint32_t sum = 0;
  for (int c = lo; c < hi; ++c) sum += ex_size(sizes[c]);
  uint32_t inc = sum;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t v = uint32_t(__shfl_up(int(inc), off, kWave));
    if (lane >= off) inc += v;
  }
  if (lane == kWave - 1) sh[wave] = inc;
  __syncthreads();
  uint32_t run = inc - sum;
  for (int w = 0; w < wave; ++w) run += sh[w];
  for (int c = lo; c < hi; ++c) {
    base[c] = run;
    run += ex_size(sizes[c]);
  }
  if (t == kExBlock - 1) base[k] = run;   // the last thread's range ends at k (it may be empty)
}

// (label, value key, index) ascending; kl = label << 32 | index
__device__ __forceinline__ bool ex_less(uint64_t kva, uint64_t kla, uint64_t kvb, uint64_t klb) {
  const uint32_t la = uint32_t(kla >> 32), lb = uint32_t(klb >> 32);
  if (la != lb) return la < lb;
  if (kva != kvb) return kva < kvb;
  return kla < klb;
}

__global__ __launch_bounds__(kExBlock) void k_ex_tile(const double* values, const int32_t* labels,
                                                      const int64_t* counters, int64_t cap, int k, uint32_t m,
                                                      int largest, const uint32_t* base, uint32_t* nan_count,
                                                      uint32_t* cursor, uint64_t* ckey, uint32_t* cidx) {
  __shared__ uint64_t skv[kExTile];
  __shared__ uint64_t skl[kExTile];
  __shared__ uint32_t soff[kExTile];
  const uint32_t cnt = ex_cnt(counters, cap);
  const uint32_t t0 = blockIdx.x * uint32_t(kExTile);
  if (t0 >= cnt) return;   // uniform
  const uint32_t t = threadIdx.x;
  uint32_t nans = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t e = t + uint32_t(h) * kExBlock, i = t0 + e;
    uint64_t kv = ~uint64_t(0), kl = ~uint64_t(0);   // pads sort behind every row
    bool nan = false;
    if (i < cnt) {
      const double v = values[i];
      const uint32_t lab = uint32_t(labels[i]);
      nan = v != v;
      if (!nan && lab < uint32_t(k)) {
        kv = ex_key(v, largest);
        kl = (uint64_t(lab) << 32) | i;
      }
    }
    nans += uint32_t(__popcll(__ballot(nan)));
    skv[e] = kv;
    skl[e] = kl;
  }
  if (nans && lane_id() == 0) atomicAdd(nan_count, nans);
  __syncthreads();
  for (uint32_t kk = 2; kk <= uint32_t(kExTile); kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      const uint32_t i = ex_pair_lo(t, j), l = i | j;
      const uint64_t va = skv[i], vb = skv[l], la = skl[i], lb = skl[l];
      if (((i & kk) == 0) != ex_less(va, la, vb, lb)) {
        skv[i] = vb;
        skv[l] = va;
        skl[i] = lb;
        skl[l] = la;
      }
      __syncthreads();
    }
  }
  // rank inside the label run, by bisection over at most m - 1 positions back;
  // a run's head takes the cursor for the whole run
  uint32_t rank[2], label[2];
  bool cand[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t p = t + uint32_t(h) * kExBlock;
    const uint32_t lab = uint32_t(skl[p] >> 32);
    label[h] = lab;
    cand[h] = lab != kNoLabel && (p < m || uint32_t(skl[p - m] >> 32) != lab);
    uint32_t r = 0;
    if (cand[h]) {
      const uint32_t back = p < m - 1 ? p : m - 1;
#pragma unroll
      for (uint32_t step = kExMaxM / 2; step > 0; step >>= 1)
        if (r + step <= back && uint32_t(skl[p - r - step] >> 32) == lab) r += step;
      if (r == 0) {
        uint32_t c = 1;
#pragma unroll
        for (uint32_t step = kExMaxM / 2; step > 0; step >>= 1)
          if (c + step <= m && p + c + step - 1 < uint32_t(kExTile) && uint32_t(skl[p + c + step - 1] >> 32) == lab)
            c += step;
        soff[p] = atomicAdd(&cursor[lab], c);
      }
    }
    rank[h] = r;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (!cand[h]) continue;
    const uint32_t p = t + uint32_t(h) * kExBlock;
    const uint32_t b = base[label[h]], end = base[label[h] + 1];
    const uint32_t pos = b + soff[p - rank[h]] + rank[h];
    if (pos < end && pos < uint32_t(cap)) {   // always, with the sizes of these labels
      ckey[pos] = skv[p];
      cidx[pos] = uint32_t(skl[p]);
    }
  }
}

__global__ __launch_bounds__(kExBlock) void k_ex_merge(const double* values, const int64_t* rows,
                                                       const int64_t* counters, int64_t cap, int k, uint32_t m,
                                                       const uint32_t* base, const uint32_t* nan_count,
                                                       const uint32_t* cursor, const uint64_t* ckey,
                                                       const uint32_t* cidx, int64_t* out) {
  __shared__ uint64_t mk[kExChunk];
  __shared__ uint32_t mi[kExChunk];
  const uint32_t cnt = ex_cnt(counters, cap);
  const uint32_t t = threadIdx.x;
  int64_t* o_counts = out + kExHead;
  int64_t* o_bits = o_counts + k;
  int64_t* o_rows = o_bits + size_t(k) * m;
  if (blockIdx.x == 0 && t == 0) {
    out[kExNNan] = int64_t(*nan_count);
    out[kExCnt] = int64_t(cnt);
    out[2] = k;
    out[3] = m;
  }
  for (int c = blockIdx.x; c < k; c += gridDim.x) {
    const uint32_t b = base[c];
    uint32_t room = base[c + 1] - b;
    if (b >= uint32_t(cap)) room = 0;
    else if (room > uint32_t(cap) - b) room = uint32_t(cap) - b;
    uint32_t nc = cursor[c];
    if (nc > room) nc = room;
    uint32_t fill = 0;   // the best so far, sorted, at the front of the chunk
    for (uint32_t pos = 0; pos < nc;) {   // uniform
      const uint32_t left = nc - pos;
      const uint32_t take = left < uint32_t(kExChunk) - fill ? left : uint32_t(kExChunk) - fill;
      const uint32_t total = fill + take;
      uint32_t P = 2;
      while (P < total) P <<= 1;
      for (uint32_t e = fill + t; e < P; e += kExBlock) {
        const bool in = e < total;
        mk[e] = in ? ckey[b + pos + (e - fill)] : ~uint64_t(0);   // pads sort behind every candidate
        mi[e] = in ? cidx[b + pos + (e - fill)] : ~0u;
      }
      __syncthreads();
      for (uint32_t kk = 2; kk <= P; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
          for (uint32_t q = t; q < (P >> 1); q += kExBlock) {
            const uint32_t i = ex_pair_lo(q, j), l = i | j;
            const uint64_t ka = mk[i], kb = mk[l];
            const uint32_t ia = mi[i], ib = mi[l];
            const bool a_first = ka < kb || (ka == kb && ia < ib);
            if (((i & kk) == 0) != a_first) {
              mk[i] = kb;
              mk[l] = ka;
              mi[i] = ib;
              mi[l] = ia;
            }
          }
          __syncthreads();
        }
      }
      fill = total < m ? total : m;
      pos += take;
    }
    for (uint32_t e = t; e < m; e += kExBlock) {
      const uint32_t idx = e < fill ? mi[e] : ~0u;
      const bool ok = idx < cnt;
      o_bits[size_t(c) * m + e] = ok ? __builtin_bit_cast(int64_t, values[idx]) : 0;
      o_rows[size_t(c) * m + e] = ok ? (rows ? rows[idx] : int64_t(idx)) : -1;
    }
    if (t == 0) o_counts[c] = fill;
    __syncthreads();   // the next cluster's chunk overwrites mk / mi
  }
}

constexpr size_t round8(size_t b) { return (b + 7) / 8 * 8; }

}  // namespace

size_t ex_scratch_words(int64_t cap, int64_t kcap, size_t out_words) {
  const size_t zero = round8(sizeof(uint32_t) * (2 + size_t(kcap)));
  const size_t base = round8(sizeof(uint32_t) * (size_t(kcap) + 1));
  const size_t key = sizeof(uint64_t) * size_t(cap), idx = round8(sizeof(uint32_t) * size_t(cap));
  return (zero + base + key + idx) / 8 + out_words;
}

ExScratch ex_scratch_carve(int64_t* buf, int64_t cap, int64_t kcap, size_t out_words) {
  ExScratch sc;
  char* p = reinterpret_cast<char*>(buf);
  sc.zero = reinterpret_cast<uint32_t*>(p);
  sc.zero_bytes = round8(sizeof(uint32_t) * (2 + size_t(kcap)));
  p += sc.zero_bytes;
  sc.base = reinterpret_cast<uint32_t*>(p);
  p += round8(sizeof(uint32_t) * (size_t(kcap) + 1));
  sc.ckey = reinterpret_cast<uint64_t*>(p);
  p += sizeof(uint64_t) * size_t(cap);
  sc.cidx = reinterpret_cast<uint32_t*>(p);
  p += round8(sizeof(uint32_t) * size_t(cap));
  sc.out = reinterpret_cast<int64_t*>(p);
  sc.cap = cap;
  sc.kcap = kcap;
  sc.out_words = out_words;
  return sc;
}

void launch_cluster_sizes(const int32_t* labels, const int64_t* counters, int64_t cap, int k, int64_t* sizes,
                          hipStream_t s) {
  if (k < 1) throw std::invalid_argument("exemplars: k must be positive");
  if (cap < 0 || cap >= (int64_t(1) << 31)) throw std::invalid_argument("exemplars: capacity out of range");
  TWTML_HIP_CHECK(hipMemsetAsync(sizes, 0, sizeof(int64_t) * size_t(k), s));
  if (cap == 0) return;
  const int g = ceil_div(cap, kBlock);
  TWTML_LAUNCH(k_ex_sizes, dim3(g > 256 ? 256 : g), dim3(kBlock), 0, s, labels, counters, cap, k, sizes);
}

void launch_cluster_select(const double* values, const int32_t* labels, const int64_t* rows, const int64_t* counters,
                           int64_t cap, int k, int m, bool largest, const int64_t* sizes, const ExScratch& sc,
                           hipStream_t s) {
  if (m < 1 || m > kExMaxM) throw std::invalid_argument("exemplars: m must be in [1, 64]");
  if (k < 1 || int64_t(k) * m > kExMaxCells) throw std::invalid_argument("exemplars: k * m must be in [1, 2^18]");
  if (cap < 0 || cap >= (int64_t(1) << 31)) throw std::invalid_argument("exemplars: capacity out of range");
  if (!sc.out || cap > sc.cap || k > sc.kcap || ex_out_words(k, m) > sc.out_words)
    throw std::invalid_argument("exemplars: the scratch is too small for this selection");
  TWTML_HIP_CHECK(hipMemsetAsync(sc.zero, 0, sizeof(uint32_t) * (2 + size_t(k)), s));
  uint32_t* nan_count = sc.zero;
  uint32_t* cursor = sc.zero + 2;
  TWTML_LAUNCH(k_ex_scan, dim3(1), dim3(kExBlock), 0, s, sizes, k, sc.base);
  if (cap > 0)
    TWTML_LAUNCH(k_ex_tile, dim3(ceil_div(cap, kExTile)), dim3(kExBlock), 0, s, values, labels, counters, cap, k,
                 uint32_t(m), largest ? 1 : 0, sc.base, nan_count, cursor, sc.ckey, sc.cidx);
  TWTML_LAUNCH(k_ex_merge, dim3(k < kExMergeGrid ? k : kExMergeGrid), dim3(kExBlock), 0, s, values, rows, counters,
               cap, k, uint32_t(m), sc.base, nan_count, cursor, sc.ckey, sc.cidx, sc.out);
}

}  // namespace twtml
