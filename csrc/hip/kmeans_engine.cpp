// KMEngine: the streaming k-means micro-batch pipeline (see kmeans.hip).
#include "kmeans_engine.h"
#include "../common/task_pool.h"
#include "trace.h"

#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <stdexcept>

#include "kmeans_kernels.h"
#include "silhouette.h"

namespace py = pybind11;

namespace twtml {

static int pad_dim(int d) {
  for (int p : {2, 4, 8, 16, 32, 64, 128})
    if (d <= p) return p;
  return d;
}

KMEngine::KMEngine(int device, const KMConfig& cfg, std::shared_ptr<Comm> comm)
    : device_(device), cfg_(cfg), comm_(std::move(comm)) {
  if (cfg_.k < 1) throw std::invalid_argument("k must be >= 1");
  // the feature kernel keeps a per-wave bigram histogram in LDS (4 waves x 4 B)
  if (cfg_.text_dims < 0 || cfg_.text_dims > 4000)
    throw std::invalid_argument("text_dims must be in [0, 4000]");
  if (cfg_.max_rows <= 0 || cfg_.max_rows >= (int64_t(1) << 31)) throw std::invalid_argument("bad max_rows");
  d_ = 2 + cfg_.text_dims;
  const char* fdp = std::getenv("TWTML_FORCE_DP");
  dist_ = comm_ && (comm_->world() > 1 || cfg_.force_dp != 0 || (fdp && fdp[0] == '1'));
  dp_ = pad_dim(d_);
  TWTML_HIP_CHECK(hipSetDevice(device_));
  compute_ = Stream(hipStreamNonBlocking);
  copy_ = Stream(hipStreamNonBlocking);
  raw_.init(cfg_.raw_slots, cfg_.max_rows, text_bytes_for_units(cfg_.max_units));
  const int64_t R = cfg_.max_rows;
  prep_.cap_rows = R;
  prep_.kept = arena_.alloc<int64_t>(size_t(R));
  prep_.nnz = arena_.alloc<int32_t>(size_t(R));
  prep_.blk = arena_.alloc<int64_t>(size_t(R / kBlock + 2));
  prep_.hist = arena_.alloc<int64_t>(kLenBuckets + 1);
  prep_.counters = arena_.alloc<int64_t>(8);
  X_ = arena_.alloc<float>(size_t(R) * size_t(dp_));
  const size_t k = size_t(cfg_.k), d = size_t(d_);
  centers_ = arena_.alloc<double>(k * d);
  weights_ = arena_.alloc<double>(k);
  sums_ = arena_.alloc<double>(k * d + k);
  sums_i_ = arena_.alloc<int64_t>(k * d + k);
  qmom_ = arena_.alloc<int64_t>(d + 1 + 4 * d);   // [d] column max | n | [d][4] sums of q and limbs
  fac64_ = arena_.alloc<double>(size_t(dp_));
  fac32_ = arena_.alloc<float>(size_t(dp_));
  blend_ = arena_.alloc<double>(2 * k);
  c32_ = arena_.alloc<float>(k * size_t(dp_));
  cnorm_ = arena_.alloc<float>(k);
  labels_ = arena_.alloc<int32_t>(size_t(R));
  order_ = arena_.alloc<int32_t>(size_t(R));
  refine_ = arena_.alloc<int32_t>(6 * size_t(R));
  frag_ = arena_.alloc<uint16_t>(km_frag_elems(cfg_.k, dp_));
  cnp_ = arena_.alloc<float>(size_t((cfg_.k + 31) / 32) * 32);
  lhist_ = arena_.alloc<int64_t>(k + 1);
  // on the compute stream: the null stream does not order against it
  TWTML_HIP_CHECK(hipMemsetAsync(centers_, 0, sizeof(double) * k * d, compute_));
  TWTML_HIP_CHECK(hipMemsetAsync(weights_, 0, sizeof(double) * k, compute_));
  upload_lower_tables(compute_, arena_, &lower_page_, &lower_blocks_);
  host_out_.alloc(sizeof(double) * (4 + d), hipHostMallocDefault);
  host_q_.alloc(sizeof(int64_t) * (d + 1 + 4 * d), hipHostMallocDefault);
  host_fac_.alloc(sizeof(double) * size_t(dp_) + sizeof(float) * size_t(dp_), hipHostMallocDefault);
  ev0_ = Event(hipEventDefault);
  ev1_ = Event(hipEventDefault);
  launch_km_centers32(centers_, cfg_.k, d_, dp_, c32_, cnorm_, compute_);
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
}

KMEngine::~KMEngine() {
  (void)hipSetDevice(device_);
  // a fault of this engine's last work surfaces here: report it (and keep it
  // for teardown_errors()) instead of leaving it to the next engine's first call
  report_teardown_error("KMEngine", device_, hipDeviceSynchronize());
  // the members release everything (streams last, see kmeans_engine.h)
}

void KMEngine::submit(const HostBatch& hb, int64_t n, int64_t bytes, int slot, const uint8_t* ext_text) {
  TraceRange tr("twtml.km.submit_h2d");
  TWTML_HIP_CHECK(hipSetDevice(device_));
  // features read only retweetCount and followersCount (scalar rows 0, 1)
  raw_.submit(hb, n, bytes, slot, copy_, 2, ext_text);
}

// K11 scaler, exact: the column max (all-reduced MAX) fixes every column's
// quantization shift, then n and the integer column sums (all-reduced SUM);
// both are the same bits on every rank and in any summation order
void KMEngine::fit_moments(bool reduce, hipStream_t s) {
  const int d = d_;
  int64_t* mx = qmom_;
  int64_t* mq = qmom_ + d;
  TWTML_HIP_CHECK(hipMemsetAsync(qmom_, 0, sizeof(int64_t) * size_t(d + 1 + 4 * d), s));
  launch_km_colmax(X_, prep_.counters, d, dp_, mx, cfg_.max_rows, s);
  if (reduce) comm_->allreduce(mx, size_t(d), ncclInt64, ncclMax, s);
  launch_km_moments_q(X_, prep_.counters, d, dp_, mx, mq, cfg_.max_rows, s);
  if (reduce) comm_->allreduce(mq, size_t(1 + 4 * d), ncclInt64, ncclSum, s);
  TWTML_HIP_CHECK(hipMemcpyAsync(host_q_, qmom_, sizeof(int64_t) * size_t(d + 1 + 4 * d), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(host_out_ + 1, prep_.counters, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
}

// batch: std_j = sqrt(M2_j / (n - 1)) (n < 2 -> 0), M2 = (n sum q^2 - (sum q)^2) / n
// in 128-bit integers; given: the caller's std_j; either way factor_j =
// std_j != 0 ? 1 / std_j : 0 (StandardScalerModel.transform); none: factor 1
void KMEngine::upload_factors(int mode, int64_t n, const double* given, std::vector<double>& std,
                              hipStream_t s) {
  const int d = d_;
  double* f64 = static_cast<double*>(host_fac_.get());
  float* f32 = reinterpret_cast<float*>(f64 + dp_);
  if (mode != kKmScalerNone) std.assign(size_t(d), 0.0);
  for (int j = 0; j < dp_; ++j) {
    double f = 0.0;
    if (j < d) {
      if (mode == kKmScalerBatch) {
        const int64_t* m = host_q_ + d + 1 + 4 * j;
        const __int128 s2 = (__int128(m[1]) << 32) + (__int128(m[2]) << 16) + __int128(m[3]);
        const __int128 num = __int128(n) * s2 - __int128(m[0]) * __int128(m[0]);
        double sd = 0.0;
        if (n > 1 && num > 0) {
          const long double var = std::ldexp(static_cast<long double>(num), 2 * km_quant_shift(host_q_[j])) /
                                  (static_cast<long double>(n) * static_cast<long double>(n - 1));
          sd = std::sqrt(static_cast<double>(var));
        }
        std[size_t(j)] = sd;
        f = sd != 0.0 ? 1.0 / sd : 0.0;
      } else if (mode == kKmScalerGiven) {
        const double sd = given[j];
        std[size_t(j)] = sd;
        f = sd != 0.0 ? 1.0 / sd : 0.0;
      } else {
        f = 1.0;
      }
    }
    f64[j] = f;
    f32[j] = float(f);
  }
  TWTML_HIP_CHECK(hipMemcpyAsync(fac64_, f64, sizeof(double) * size_t(dp_), hipMemcpyHostToDevice, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(fac32_, f32, sizeof(float) * size_t(dp_), hipMemcpyHostToDevice, s));
}

void KMEngine::ensure_score() {
  if (dist2_) return;
  const size_t R = size_t(cfg_.max_rows);
  cost_parts_ = R / size_t(km_cost_shape(dp_).rows_per_wg) + 1;
  dist2_ = arena_.alloc<double>(R);
  cost_part_ = arena_.alloc<double>(cost_parts_ + 1);
  score_host_.alloc(R * (sizeof(int64_t) + sizeof(double) + sizeof(int32_t)) + sizeof(double) +
                        sizeof(int64_t) * size_t(cfg_.k),
                    hipHostMallocDefault);
}

int64_t KMEngine::score_kernels(const char* who, int slot, bool apply_filter, int scaler_mode, const double* std,
                                KMScoreResult& res, double** cost_out) {
  const std::string w(who);
  if (scaler_mode < kKmScalerBatch || scaler_mode > kKmScalerNone)
    throw std::invalid_argument(w + ": unknown scaler mode");
  if (scaler_mode == kKmScalerGiven && !std) throw std::invalid_argument(w + ": the given scaler needs std");
  TWTML_HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = compute_;
  const int k = cfg_.k, d = d_;
  ensure_score();
  res.sizes.assign(size_t(k), 0);
  const DevRawBatch b = raw_.acquire(slot, s);
  res.n_raw = b.n;
  TWTML_HIP_CHECK(hipEventRecord(ev0_, s));
  FeaturizeParams fp{1, 0, apply_filter ? 1 : 0, 0, 0, 0, 0};   // the training filter, or every row
  TWTML_HIP_CHECK(hipMemsetAsync(prep_.counters, 0, 8 * sizeof(int64_t), s));
  launch_filter_only(b, prep_, fp, s);
  launch_km_features(b, prep_.kept, prep_.counters, X_, dp_, cfg_.text_dims, lower_page_,
                     lower_blocks_, cfg_.max_rows, s);
  raw_.release_slot(slot, s);
  if (scaler_mode == kKmScalerBatch) {
    fit_moments(false, s);   // never a collective: a DP rank fits on its own shard
  } else {
    TWTML_HIP_CHECK(hipMemcpyAsync(host_out_ + 1, prep_.counters, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipStreamSynchronize(s));
  }
  int64_t n;
  std::memcpy(&n, host_out_ + 1, sizeof(int64_t));
  if (n < 0 || n > b.n || n > cfg_.max_rows || (!apply_filter && n != b.n))
    throw std::runtime_error(w + ": kept-row count out of range");
  res.n_scored = n;
  if (n == 0) {   // nothing to assign: no assign or cost launch
    TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
    TWTML_HIP_CHECK(hipStreamSynchronize(s));
    TWTML_HIP_CHECK(hipEventElapsedTime(&res.ms, ev0_, ev1_));
    return 0;
  }
  upload_factors(scaler_mode, n, std, res.std, s);
  auto* refine_cnt = reinterpret_cast<unsigned long long*>(prep_.counters + 5);
  launch_km_assign(X_, fac32_, fac64_, prep_.counters, c32_, cnorm_, centers_, k, d, dp_, labels_,
                   refine_, refine_cnt, frag_, cnp_, cfg_.max_rows, cfg_.mfma != 0, cfg_.mfma == 1, s);
  double* cost = cost_part_ + cost_parts_;
  launch_km_cost(X_, fac64_, labels_, centers_, prep_.counters, n, k, d, dp_, dist2_, cost_part_, cost,
                 lhist_, s);
  *cost_out = cost;
  return n;
}

KMScoreResult KMEngine::score(int slot, bool apply_filter, int scaler_mode, const double* std) {
  TraceRange tr("twtml.km.score");
  KMScoreResult res;
  double* cost = nullptr;
  const int64_t n = score_kernels("score()", slot, apply_filter, scaler_mode, std, res, &cost);
  if (n == 0) return res;
  hipStream_t s = compute_;
  const int k = cfg_.k;
  TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
  const size_t R = size_t(cfg_.max_rows), un = size_t(n);
  auto* h_rows = static_cast<int64_t*>(score_host_.get());
  auto* h_dist2 = reinterpret_cast<double*>(h_rows + R);
  double* h_cost = h_dist2 + R;
  auto* h_sizes = reinterpret_cast<int64_t*>(h_cost + 1);
  auto* h_labels = reinterpret_cast<int32_t*>(h_sizes + k);
  TWTML_HIP_CHECK(hipMemcpyAsync(h_rows, prep_.kept, sizeof(int64_t) * un, hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_dist2, dist2_, sizeof(double) * un, hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_cost, cost, sizeof(double), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_sizes, lhist_, sizeof(int64_t) * size_t(k), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_labels, labels_, sizeof(int32_t) * un, hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  res.rows = h_rows;
  res.dist2 = h_dist2;
  res.labels = h_labels;
  res.cost = *h_cost;
  res.sizes.assign(h_sizes, h_sizes + k);
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.ms, ev0_, ev1_));
  return res;
}

void KMEngine::ensure_top() {
  if (top_sc_.out) return;
  top_host_.alloc(sizeof(int64_t) * (top_out_words(kTopNMax) + 1 + size_t(cfg_.k)), hipHostMallocDefault);
  top_sc_ = top_scratch_carve(arena_.alloc<int64_t>(top_scratch_words()));
}

KMTopResult KMEngine::top(int slot, bool apply_filter, int scaler_mode, const double* std, int n, bool largest) {
  if (n < 1 || n > kTopNMax)
    throw std::invalid_argument("top(): n must be in [1, " + std::to_string(kTopNMax) + "]; use score() for every row");
  TraceRange tr("twtml.km.top");
  KMTopResult res;
  double* cost = nullptr;
  const int64_t ns = score_kernels("top()", slot, apply_filter, scaler_mode, std, res.batch, &cost);
  res.top.n_raw = res.batch.n_raw;
  if (ns == 0) return res;
  ensure_top();
  hipStream_t s = compute_;
  const size_t k = size_t(cfg_.k);
  launch_top_select(dist2_, prep_.kept, labels_, prep_.counters, cfg_.max_rows, n, largest, top_sc_, s);
  TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
  int64_t* h = top_host_.get();
  int64_t* h_cost = h + top_out_words(kTopNMax);
  int64_t* h_sizes = h_cost + 1;
  TWTML_HIP_CHECK(hipMemcpyAsync(h, top_sc_.out, sizeof(int64_t) * top_out_words(n), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_cost, cost, sizeof(double), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_sizes, lhist_, sizeof(int64_t) * k, hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  TopResult& t = res.top;
  t.n_scored = h[kTopCnt];
  t.n_top = h[kTopNTop];
  t.n_nan = h[kTopNNan];
  if (t.n_scored != ns || t.n_top < 0 || t.n_top > n || t.n_nan < 0 || t.n_top + t.n_nan > ns)
    throw std::runtime_error("top(): the result block's counts are out of range");
  t.bits = h + kTopHead;
  t.rows = h + kTopHead + n;
  t.payload = h + kTopHead + 2 * size_t(n);
  std::memcpy(&res.batch.cost, h_cost, sizeof(double));
  res.batch.sizes.assign(h_sizes, h_sizes + k);
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.batch.ms, ev0_, ev1_));
  t.top_ms = res.batch.ms;
  return res;
}

// ---------------------------------------------------------------------------
// Exemplars (exemplars.hip): score()'s pass, then one top-m per cluster.
// ---------------------------------------------------------------------------
static void check_ex(const char* who, int64_t k, int m) {
  if (m < 1 || m > kExMaxM || k < 1 || k * m > kExMaxCells)
    throw std::invalid_argument(std::string(who) + ": m must be in [1, " + std::to_string(kExMaxM) +
                                "] and k * m at most " + std::to_string(kExMaxCells) + "; use score() for every row");
}

void KMEngine::ensure_ex(int64_t kcap, size_t out_words) {
  if (ex_sc_.out && ex_sc_.kcap >= kcap && ex_sc_.out_words >= out_words) return;
  kcap = std::max(kcap, ex_sc_.kcap);   // debug_cluster_select() with a larger k: never smaller than before
  out_words = std::max(out_words, ex_sc_.out_words);
  if (!ex_ev_) ex_ev_ = Event(hipEventDefault);
  const size_t host_words = out_words + 1 + size_t(cfg_.k);
  if (host_words > ex_host_words_) {
    ex_host_.alloc(sizeof(int64_t) * host_words, hipHostMallocDefault);
    ex_host_words_ = host_words;
  }
  ex_sc_ = ExScratch{};
  arena_.grow(ex_buf_, ex_scratch_words(cfg_.max_rows, kcap, out_words), compute_);
  ex_sc_ = ex_scratch_carve(ex_buf_, cfg_.max_rows, kcap, out_words);
}

KMExemplarResult KMEngine::ex_result(int k, int m, const double* cost) {
  hipStream_t s = compute_;
  const size_t words = ex_out_words(k, m);
  int64_t* h = ex_host_.get();
  int64_t* h_cost = h + words;
  int64_t* h_sizes = h_cost + 1;
  TWTML_HIP_CHECK(hipMemcpyAsync(h, ex_sc_.out, sizeof(int64_t) * words, hipMemcpyDeviceToHost, s));
  if (cost) {
    TWTML_HIP_CHECK(hipMemcpyAsync(h_cost, cost, sizeof(double), hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_sizes, lhist_, sizeof(int64_t) * size_t(cfg_.k), hipMemcpyDeviceToHost, s));
  }
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  KMExemplarResult res;
  res.k = k;
  res.m = m;
  res.n_nan = h[kExNNan];
  res.batch.n_scored = h[kExCnt];
  res.counts = h + kExHead;
  res.bits = res.counts + k;
  res.rows = res.bits + size_t(k) * size_t(m);
  if (res.n_nan < 0 || res.n_nan > res.batch.n_scored)
    throw std::runtime_error("exemplars(): the result block's counts are out of range");
  if (cost) {
    std::memcpy(&res.batch.cost, h_cost, sizeof(double));
    res.batch.sizes.assign(h_sizes, h_sizes + cfg_.k);
  }
  return res;
}

KMExemplarResult KMEngine::exemplars(int slot, bool apply_filter, int scaler_mode, const double* std, int m,
                                     bool largest) {
  check_ex("exemplars()", cfg_.k, m);
  TraceRange tr("twtml.km.exemplars");
  KMScoreResult batch;
  double* cost = nullptr;
  const int64_t ns = score_kernels("exemplars()", slot, apply_filter, scaler_mode, std, batch, &cost);
  if (ns == 0) {
    KMExemplarResult res;
    res.batch = std::move(batch);
    res.k = cfg_.k;
    res.m = m;
    res.ex_ms = res.batch.ms;
    return res;
  }
  const int64_t m_most = std::min<int64_t>(kExMaxM, kExMaxCells / cfg_.k);
  ensure_ex(cfg_.k, ex_out_words(cfg_.k, int(m_most)));
  hipStream_t s = compute_;
  TWTML_HIP_CHECK(hipEventRecord(ex_ev_, s));
  launch_cluster_select(dist2_, labels_, prep_.kept, prep_.counters, ns, cfg_.k, m, largest, lhist_, ex_sc_, s);
  TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
  KMExemplarResult res = ex_result(cfg_.k, m, cost);
  if (res.batch.n_scored != ns) throw std::runtime_error("exemplars(): the result block's row count is out of range");
  res.batch.n_raw = batch.n_raw;
  res.batch.std = std::move(batch.std);
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.batch.ms, ev0_, ev1_));
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.sel_ms, ex_ev_, ev1_));
  res.ex_ms = res.batch.ms;
  return res;
}

KMExemplarResult KMEngine::debug_cluster_select(const double* values, const int32_t* labels, const int64_t* rows,
                                                int64_t count, int k, int m, bool largest) {
  check_ex("debug_cluster_select()", k, m);
  if (count < 0 || count > cfg_.max_rows)
    throw std::invalid_argument("debug_cluster_select(): more values than max_rows");
  TWTML_HIP_CHECK(hipSetDevice(device_));
  // the buffers of a scoring pass stand in for its outputs: dist2_ / labels_ /
  // the kept row ids / the row counter on the device, score()'s pinned block
  // as the staging of the caller's arrays (what the last score() left there is
  // overwritten); only the sizes of the caller's k are the entry's own
  ensure_score();
  ensure_ex(k, ex_out_words(k, m));
  if (k > ex_dbg_k_) {
    arena_.grow(ex_dbg_sizes_, size_t(k), compute_);
    ex_dbg_k_ = k;
  }
  hipStream_t s = compute_;
  const size_t R = size_t(cfg_.max_rows), un = size_t(count);
  auto* h_rows = static_cast<int64_t*>(score_host_.get());
  auto* h_vals = reinterpret_cast<double*>(h_rows + R);
  auto* h_labels = reinterpret_cast<int32_t*>(reinterpret_cast<int64_t*>(h_vals + R + 1) + cfg_.k);
  int64_t* d_sizes = ex_dbg_sizes_;
  double* dv = dist2_;
  int64_t* dr = prep_.kept;
  int32_t* dl = labels_;
  std::memcpy(host_out_ + 1, &count, sizeof(int64_t));
  TWTML_HIP_CHECK(hipMemsetAsync(prep_.counters, 0, 8 * sizeof(int64_t), s));
  TWTML_HIP_CHECK(hipMemcpyAsync(prep_.counters, host_out_ + 1, sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (count > 0) {
    std::memcpy(h_vals, values, sizeof(double) * un);
    std::memcpy(h_labels, labels, sizeof(int32_t) * un);
    TWTML_HIP_CHECK(hipMemcpyAsync(dv, h_vals, sizeof(double) * un, hipMemcpyHostToDevice, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(dl, h_labels, sizeof(int32_t) * un, hipMemcpyHostToDevice, s));
    if (rows) {
      std::memcpy(h_rows, rows, sizeof(int64_t) * un);
      TWTML_HIP_CHECK(hipMemcpyAsync(dr, h_rows, sizeof(int64_t) * un, hipMemcpyHostToDevice, s));
    }
  }
  launch_cluster_sizes(dl, prep_.counters, count, k, d_sizes, s);
  TWTML_HIP_CHECK(hipEventRecord(ex_ev_, s));
  launch_cluster_select(dv, dl, rows ? dr : nullptr, prep_.counters, count, k, m, largest, d_sizes, ex_sc_, s);
  TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
  KMExemplarResult res = ex_result(k, m, nullptr);
  res.batch.n_raw = count;
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.sel_ms, ex_ev_, ev1_));
  res.ex_ms = res.sel_ms;
  return res;
}

void KMEngine::ensure_sil() {
  if (sil_mean_) return;
  const size_t R = size_t(cfg_.max_rows), k = size_t(cfg_.k), d = size_t(d_);
  sil_mean_ = arena_.alloc<double>(k * d);
  sil_dev2_ = arena_.alloc<double>(R);
  sil_part_ = arena_.alloc<double>(cost_parts_ + 1);
  sil_W_ = arena_.alloc<double>(k);
  sil_V_ = arena_.alloc<double>(k);
  sil_mu32_ = arena_.alloc<float>(k * size_t(dp_));
  sil_B_ = arena_.alloc<float>(k);
  sil_wacc_ = arena_.alloc<unsigned long long>(2 * k);
  sil_hist_ = arena_.alloc<int64_t>(k + 1);
  sil_sizes_ = arena_.alloc<int64_t>(k);
  sil_words_ = arena_.alloc<int64_t>(sil_words(cfg_.k));
  sil_nb_ = arena_.alloc<int32_t>(R);
  sil_a_ = arena_.alloc<double>(R);
  sil_b_ = arena_.alloc<double>(R);
  sil_s_ = arena_.alloc<double>(R);
  sil_host_.alloc(sizeof(int64_t) * (sil_words(cfg_.k) + 1 + k) + R * (sizeof(int64_t) + 3 * sizeof(double) +
                                                                         2 * sizeof(int32_t)),
                  hipHostMallocDefault);
}

KMSilResult KMEngine::silhouette(int slot, bool apply_filter, int scaler_mode, const double* std, bool per_row) {
  TraceRange tr("twtml.km.silhouette");
  KMSilResult res;
  res.per_row = per_row;
  const int k = cfg_.k, d = d_;
  res.n.assign(size_t(k), 0);
  res.s_fix.assign(size_t(k), 0);
  double* cost = nullptr;
  const int64_t n = score_kernels("silhouette()", slot, apply_filter, scaler_mode, std, res.batch, &cost);
  if (n == 0) return res;
  hipStream_t s = compute_;
  ensure_sil();
  const size_t R = size_t(cfg_.max_rows), un = size_t(n), nw = sil_words(k);
  auto* h_words = static_cast<int64_t*>(sil_host_.get());
  auto* h_cost = reinterpret_cast<double*>(h_words + nw);
  auto* h_sizes = reinterpret_cast<int64_t*>(h_cost + 1);
  auto* h_rows = h_sizes + k;
  auto* h_a = reinterpret_cast<double*>(h_rows + R);
  double *h_b = h_a + R, *h_s = h_b + R;
  auto* h_labels = reinterpret_cast<int32_t*>(h_s + R);
  int32_t* h_nb = h_labels + R;
  // the sizes decide what runs: fewer than two non-empty clusters is undefined
  TWTML_HIP_CHECK(hipMemcpyAsync(h_cost, cost, sizeof(double), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipMemcpyAsync(h_sizes, lhist_, sizeof(int64_t) * size_t(k), hipMemcpyDeviceToHost, s));
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  res.batch.cost = *h_cost;
  res.batch.sizes.assign(h_sizes, h_sizes + k);
  int64_t total = 0;
  for (int c = 0; c < k; ++c) {
    total += h_sizes[c];
    res.nonempty += h_sizes[c] > 0;
  }
  if (total != n) throw std::runtime_error("silhouette(): labels outside the model's clusters (NaN centres?)");
  if (n > kSilMaxRows)
    throw std::invalid_argument("silhouette(): a batch of more than " + std::to_string(kSilMaxRows) + " scored rows");
  const bool defined = res.nonempty >= 2;
  if (defined) {
    int64_t* mx = qmom_;   // the batch scaler left the column maxima here; the other modes fit them now
    if (scaler_mode != kKmScalerBatch) {
      TWTML_HIP_CHECK(hipMemsetAsync(mx, 0, sizeof(int64_t) * size_t(d), s));
      launch_km_colmax(X_, prep_.counters, d, dp_, mx, cfg_.max_rows, s);
    }
    double* counts = sums_ + size_t(k) * d;
    TWTML_HIP_CHECK(hipMemsetAsync(sums_i_, 0, sizeof(int64_t) * (size_t(k) * d + k), s));
    launch_km_cluster_sums(X_, mx, labels_, prep_.counters, k, d, dp_, sil_hist_, order_, sums_i_, cfg_.max_rows, s,
                           &scan_excl_launch);
    launch_km_sums_f64(sums_i_, mx, fac64_, k, d, sums_, counts, s);
    launch_sil_means(sums_, counts, k, d, sil_mean_, s);
    launch_km_cost(X_, fac64_, labels_, sil_mean_, prep_.counters, n, k, d, dp_, sil_dev2_, sil_part_,
                   sil_part_ + cost_parts_, sil_sizes_, s);
    launch_sil_stats(sil_dev2_, labels_, n, k, d, dp_, sil_mean_, sil_sizes_, sil_wacc_, sil_wacc_ + k, sil_W_,
                     sil_V_, sil_mu32_, sil_B_, s);
    TWTML_HIP_CHECK(hipMemsetAsync(sil_words_, 0, sizeof(int64_t) * nw, s));
    launch_sil_neighbor(X_, fac32_, fac64_, labels_, sil_dev2_, n, k, d, dp_, sil_mean_, sil_mu32_, sil_B_, sil_V_,
                        sil_W_, sil_sizes_, cfg_.mfma != 0, sil_words_, per_row ? sil_nb_ : nullptr, sil_a_, sil_b_,
                        sil_s_, s);
    TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_words, sil_words_, sizeof(int64_t) * nw, hipMemcpyDeviceToHost, s));
  } else {
    TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
    if (per_row) {   // no neighbour, a = b = s = 0
      TWTML_HIP_CHECK(hipMemsetAsync(sil_nb_, 0xff, sizeof(int32_t) * un, s));
      for (double* p : {sil_a_, sil_b_, sil_s_}) TWTML_HIP_CHECK(hipMemsetAsync(p, 0, sizeof(double) * un, s));
    }
  }
  if (per_row) {
    TWTML_HIP_CHECK(hipMemcpyAsync(h_rows, prep_.kept, sizeof(int64_t) * un, hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_labels, labels_, sizeof(int32_t) * un, hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_nb, sil_nb_, sizeof(int32_t) * un, hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_a, sil_a_, sizeof(double) * un, hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_b, sil_b_, sizeof(double) * un, hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipMemcpyAsync(h_s, sil_s_, sizeof(double) * un, hipMemcpyDeviceToHost, s));
  }
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.batch.ms, ev0_, ev1_));
  if (defined) {
    res.n.assign(h_words, h_words + k);
    res.s_fix.assign(h_words + k, h_words + 2 * k);
    res.n_single = h_words[2 * k];
    int64_t counted = 0;
    for (int c = 0; c < k; ++c) counted += res.n[size_t(c)];
    if (counted != n || res.n_single < 0 || res.n_single > n)
      throw std::runtime_error("silhouette(): the result words' counts are out of range");
  } else {
    res.n_undefined = n;
  }
  if (per_row) {
    res.rows = h_rows;
    res.labels = h_labels;
    res.neighbor = h_nb;
    res.a = h_a;
    res.b = h_b;
    res.s = h_s;
  }
  return res;
}

KMResult KMEngine::process(int slot, bool want_labels) {
  TraceRange tr("twtml.km.batch");
  TWTML_HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = compute_;
  const int k = cfg_.k, d = d_;
  KMResult res;
  const DevRawBatch b = raw_.acquire(slot, s);
  res.n_raw = b.n;
  TWTML_HIP_CHECK(hipEventRecord(ev0_, s));
  FeaturizeParams fp{1, 0, 1, 0, 0, 0, 0};   // filter: isRetweet only (KMeans.scala:77-80)
  TWTML_HIP_CHECK(hipMemsetAsync(prep_.counters, 0, 8 * sizeof(int64_t), s));
  launch_filter_only(b, prep_, fp, s);
  launch_km_features(b, prep_.kept, prep_.counters, X_, dp_, cfg_.text_dims, lower_page_,
                     lower_blocks_, cfg_.max_rows, s);
  raw_.release_slot(slot, s);
  int64_t* mx = qmom_;
  fit_moments(dist_, s);
  res.n_global = host_q_[d];
  int64_t nl;
  std::memcpy(&nl, host_out_ + 1, sizeof(int64_t));
  res.n_local = nl;
  if (res.n_global == 0) {                  // if (rdd.count > 0) { ... }
    TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
    TWTML_HIP_CHECK(hipStreamSynchronize(s));
    return res;
  }
  upload_factors(cfg_.scale ? kKmScalerBatch : kKmScalerNone, res.n_global, nullptr, res.std, s);
  // K8 assignment with the current centres, K9 sums, K10 update.  The
  // near-tie lists in refine_, their counts in counters[5..6].
  auto* refine_cnt = reinterpret_cast<unsigned long long*>(prep_.counters + 5);
  launch_km_assign(X_, fac32_, fac64_, prep_.counters, c32_, cnorm_, centers_, k, d, dp_, labels_,
                   refine_, refine_cnt, frag_, cnp_, cfg_.max_rows, cfg_.mfma != 0, cfg_.mfma == 1, s);
  // TWTML_DEBUG_KM=1: per-assignment near-tie counts (synchronises the stream)
  static const bool debug = std::getenv("TWTML_DEBUG_KM") != nullptr;
  auto debug_refine = [&](const char* what) {
    if (!debug) return;
    unsigned long long c[2];
    TWTML_HIP_CHECK(hipMemcpyAsync(c, refine_cnt, sizeof(c), hipMemcpyDeviceToHost, s));
    TWTML_HIP_CHECK(hipStreamSynchronize(s));
    std::fprintf(stderr, "[km] %s: n=%lld refine full=%llu candidates=%llu\n", what,
                 static_cast<long long>(res.n_local), c[0], c[1]);
  };
  debug_refine("update");
  TWTML_HIP_CHECK(hipMemsetAsync(sums_i_, 0, sizeof(int64_t) * (size_t(k) * d + k), s));
  launch_km_cluster_sums(X_, mx, labels_, prep_.counters, k, d, dp_, lhist_, order_, sums_i_, cfg_.max_rows, s,
                         &scan_excl_launch);
  if (dist_) comm_->allreduce(sums_i_, size_t(k) * d + k, ncclInt64, ncclSum, s);
  launch_km_sums_f64(sums_i_, mx, fac64_, k, d, sums_, sums_ + size_t(k) * d, s);
  launch_km_update(centers_, weights_, sums_, sums_ + size_t(k) * d, k, d, cfg_.decay,
                   cfg_.points_unit != 0, blend_, c32_, cnorm_, dp_, s);
  if (want_labels)   // KMeans.scala:113 predicts with the updated model
    launch_km_assign(X_, fac32_, fac64_, prep_.counters, c32_, cnorm_, centers_, k, d, dp_, labels_,
                     refine_, refine_cnt, frag_, cnp_, cfg_.max_rows, cfg_.mfma != 0, cfg_.mfma == 1, s);
  if (want_labels) debug_refine("predict");
  TWTML_HIP_CHECK(hipEventRecord(ev1_, s));
  if (want_labels && res.n_local > 0) {
    res.labels.resize(size_t(res.n_local));
    TWTML_HIP_CHECK(hipMemcpyAsync(res.labels.data(), labels_, sizeof(int32_t) * size_t(res.n_local),
                                   hipMemcpyDeviceToHost, s));
  }
  TWTML_HIP_CHECK(hipStreamSynchronize(s));
  if (comm_) comm_->check_async();
  TWTML_HIP_CHECK(hipEventElapsedTime(&res.ms, ev0_, ev1_));
  return res;
}

void KMEngine::set_state(const double* centers, const double* weights) {
  TWTML_HIP_CHECK(hipSetDevice(device_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  // stream-ordered and complete on return (a pageable hipMemcpy may return
  // before its DMA lands, unordered against the non-blocking compute stream)
  TWTML_HIP_CHECK(hipMemcpyAsync(centers_, centers, sizeof(double) * size_t(cfg_.k) * d_, hipMemcpyHostToDevice,
                                 compute_));
  TWTML_HIP_CHECK(hipMemcpyAsync(weights_, weights, sizeof(double) * size_t(cfg_.k), hipMemcpyHostToDevice,
                                 compute_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  launch_km_centers32(centers_, cfg_.k, d_, dp_, c32_, cnorm_, compute_);
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
}

std::vector<int32_t> KMEngine::debug_labels() const {
  TWTML_HIP_CHECK(hipSetDevice(device_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  int64_t n = 0;
  TWTML_HIP_CHECK(hipMemcpy(&n, prep_.counters, sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> out(size_t(std::max<int64_t>(n, 0)));
  if (n > 0) TWTML_HIP_CHECK(hipMemcpy(out.data(), labels_, sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost));
  return out;
}

std::vector<float> KMEngine::debug_features() const {
  TWTML_HIP_CHECK(hipSetDevice(device_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  int64_t n = 0;
  TWTML_HIP_CHECK(hipMemcpy(&n, prep_.counters, sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<float> out(size_t(std::max<int64_t>(n, 0)) * size_t(dp_));
  if (n > 0) TWTML_HIP_CHECK(hipMemcpy(out.data(), X_, sizeof(float) * out.size(), hipMemcpyDeviceToHost));
  return out;
}

void KMEngine::get_state(double* centers, double* weights) const {
  TWTML_HIP_CHECK(hipSetDevice(device_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  TWTML_HIP_CHECK(hipMemcpy(centers, centers_, sizeof(double) * size_t(cfg_.k) * d_, hipMemcpyDeviceToHost));
  TWTML_HIP_CHECK(hipMemcpy(weights, weights_, sizeof(double) * size_t(cfg_.k), hipMemcpyDeviceToHost));
}

void KMEngine::synchronize() {
  TWTML_HIP_CHECK(hipSetDevice(device_));
  TWTML_HIP_CHECK(hipStreamSynchronize(compute_));
  TWTML_HIP_CHECK(hipStreamSynchronize(copy_));
}

// ---------------------------------------------------------------------------
void bind_kmeans(py::module_& m) {
  py::class_<KMEngine, std::shared_ptr<KMEngine>>(m, "KMEngine")
      .def(py::init([](int device, const py::dict& d, std::shared_ptr<Comm> comm) {
             KMConfig c;
#define GET(name, type) if (d.contains(#name)) c.name = d[#name].cast<type>();
             GET(k, int32_t) GET(text_dims, int32_t) GET(decay, double) GET(points_unit, int32_t)
             GET(scale, int32_t) GET(mfma, int32_t) GET(max_rows, int64_t) GET(max_units, int64_t)
             GET(force_dp, int32_t) GET(raw_slots, int32_t)
#undef GET
             py::gil_scoped_release nogil;
             return std::make_shared<KMEngine>(device, c, comm);
           }),
           py::arg("device"), py::arg("config"), py::arg("comm") = nullptr)
      .def("submit", [](KMEngine& e, const HostBatch& hb, int64_t n, int64_t bytes, int slot, uintptr_t ext_text) {
        py::gil_scoped_release nogil;
        e.submit(hb, n, bytes, slot, reinterpret_cast<const uint8_t*>(ext_text));
      }, py::arg("host_batch"), py::arg("n"), py::arg("bytes"), py::arg("slot"), py::arg("ext_text") = 0)
      .def("discard", [](KMEngine& e, int slot) {
        py::gil_scoped_release nogil;
        e.discard(slot);
      }, py::arg("slot"), "forget a submitted batch that will not be processed")
      .def_property_readonly("h2d_bytes", &KMEngine::h2d_bytes, "host-to-device bytes submitted so far")
      .def_property_readonly("raw_slots", &KMEngine::raw_slots, "device raw-batch slots")
      .def("process", [](KMEngine& e, int slot, bool want_labels) {
        KMResult r;
        {
          py::gil_scoped_release nogil;
          r = e.process(slot, want_labels);
        }
        py::dict out;
        out["n_raw"] = r.n_raw;
        out["n_local"] = r.n_local;
        out["n"] = r.n_global;
        out["std"] = r.std;
        out["ms"] = r.ms;
        if (!r.labels.empty())
          out["pred"] = py::array_t<int32_t>(py::ssize_t(r.labels.size()), r.labels.data());
        else
          out["pred"] = py::none();
        return out;
      }, py::arg("slot"), py::arg("want_labels") = false)
      .def("score", [](KMEngine& e, int slot, bool apply_filter, int scaler_mode,
                       std::optional<py::array_t<double, py::array::c_style | py::array::forcecast>> std) {
        if (scaler_mode == kKmScalerGiven && (!std || std->size() != e.d()))
          throw std::invalid_argument("score(): the given scaler needs d stds");
        KMScoreResult r;
        {
          const double* sp = std ? std->data() : nullptr;
          py::gil_scoped_release nogil;
          r = e.score(slot, apply_filter, scaler_mode, sp);
        }
        // copies owned by the caller (the engine's pinned buffer is reused)
        py::array_t<int64_t> rows(r.n_scored);
        py::array_t<int32_t> pred(r.n_scored);
        py::array_t<double> dist2(r.n_scored);
        if (r.n_scored > 0) {
          // 1 MB pieces on the host pool: a fresh array's first-touch page
          // faults make one thread's copy of 20 B x 1M rows longer than the kernels
          struct Part { char* dst; const char* src; size_t bytes; };
          const size_t n = size_t(r.n_scored);
          const Part parts[3] = {{reinterpret_cast<char*>(rows.mutable_data()), reinterpret_cast<const char*>(r.rows), 8 * n},
                                 {reinterpret_cast<char*>(dist2.mutable_data()), reinterpret_cast<const char*>(r.dist2), 8 * n},
                                 {reinterpret_cast<char*>(pred.mutable_data()), reinterpret_cast<const char*>(r.labels), 4 * n}};
          constexpr size_t kPiece = size_t(1) << 20;
          int first[4] = {0, 0, 0, 0};
          for (int p = 0; p < 3; ++p) first[p + 1] = first[p] + int((parts[p].bytes + kPiece - 1) / kPiece);
          py::gil_scoped_release nogil;
          TaskPool::get().run(first[3], [&](int t) {
            const int p = t >= first[2] ? 2 : (t >= first[1] ? 1 : 0);
            const size_t off = size_t(t - first[p]) * kPiece;
            std::memcpy(parts[p].dst + off, parts[p].src + off, std::min(kPiece, parts[p].bytes - off));
          });
        }
        py::dict out;
        out["n_raw"] = r.n_raw;
        out["n_scored"] = r.n_scored;
        out["rows"] = rows;
        out["pred"] = pred;
        out["dist2"] = dist2;
        out["cost"] = r.cost;
        out["sizes"] = py::array_t<int64_t>(py::ssize_t(r.sizes.size()), r.sizes.data());
        out["std"] = py::array_t<double>(py::ssize_t(r.std.size()), r.std.data());
        out["score_ms"] = r.ms;
        return out;
      }, py::arg("slot"), py::arg("apply_filter") = true, py::arg("scaler_mode") = 0, py::arg("std") = py::none(),
         "inference only: labels, squared distances, cost and cluster sizes of the batch in `slot` under the "
         "current model; scaler_mode 0 per-batch fit, 1 the given std[d], 2 none")
      .def("top", [](KMEngine& e, int slot, bool apply_filter, int scaler_mode,
                     std::optional<py::array_t<double, py::array::c_style | py::array::forcecast>> std, int n,
                     bool largest) {
        if (scaler_mode == kKmScalerGiven && (!std || std->size() != e.d()))
          throw std::invalid_argument("top(): the given scaler needs d stds");
        KMTopResult r;
        {
          const double* sp = std ? std->data() : nullptr;
          py::gil_scoped_release nogil;
          r = e.top(slot, apply_filter, scaler_mode, sp, n, largest);
        }
        py::dict out = top_dict(r.top);
        out["n_scored"] = r.batch.n_scored;
        out["cost"] = r.batch.cost;
        out["sizes"] = py::array_t<int64_t>(py::ssize_t(r.batch.sizes.size()), r.batch.sizes.data());
        out["std"] = py::array_t<double>(py::ssize_t(r.batch.std.size()), r.batch.std.data());
        return out;
      }, py::arg("slot"), py::arg("apply_filter") = true, py::arg("scaler_mode") = 0, py::arg("std") = py::none(),
         py::arg("n") = 1, py::arg("largest") = true,
         "inference only: the n rows farthest from (largest) or closest to their centres, selected on the device: "
         "rows, values (squared distances), payload (labels), with the batch's cost, sizes and std")
      .def("exemplars", [](KMEngine& e, int slot, bool apply_filter, int scaler_mode,
                           std::optional<py::array_t<double, py::array::c_style | py::array::forcecast>> std, int m,
                           bool largest) {
        if (scaler_mode == kKmScalerGiven && (!std || std->size() != e.d()))
          throw std::invalid_argument("exemplars(): the given scaler needs d stds");
        KMExemplarResult r;
        {
          const double* sp = std ? std->data() : nullptr;
          py::gil_scoped_release nogil;
          r = e.exemplars(slot, apply_filter, scaler_mode, sp, m, largest);
        }
        py::dict out = exemplar_dict(r);
        out["cost"] = r.batch.cost;
        out["sizes"] = py::array_t<int64_t>(py::ssize_t(r.batch.sizes.size()), r.batch.sizes.data());
        out["std"] = py::array_t<double>(py::ssize_t(r.batch.std.size()), r.batch.std.data());
        return out;
      }, py::arg("slot"), py::arg("apply_filter") = true, py::arg("scaler_mode") = 0, py::arg("std") = py::none(),
         py::arg("m") = 1, py::arg("largest") = false,
         "inference only: per cluster, the m rows closest to (largest: farthest from) their centre, selected on the "
         "device: counts[k], rows[k, m], values[k, m] (squared distances), n_nan, with the batch's cost, sizes and std")
      .def("debug_cluster_select",
           [](KMEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> values,
              py::array_t<int32_t, py::array::c_style | py::array::forcecast> labels,
              std::optional<py::array_t<int64_t, py::array::c_style | py::array::forcecast>> rows, int k, int m,
              bool largest) {
             if (values.ndim() != 1 || labels.ndim() != 1 || labels.size() != values.size() ||
                 (rows && (rows->ndim() != 1 || rows->size() != values.size())))
               throw std::invalid_argument(
                   "debug_cluster_select(): values, labels and rows are 1-d arrays of one length");
             for (py::ssize_t i = 0; i < labels.size(); ++i)
               if (labels.data()[i] < 0 || labels.data()[i] >= k)
                 throw std::invalid_argument("debug_cluster_select(): labels must lie in [0, k)");
             KMExemplarResult r;
             {
               const double* v = values.data();
               const int32_t* l = labels.data();
               const int64_t* rp = rows ? rows->data() : nullptr;
               const int64_t count = values.size();
               py::gil_scoped_release nogil;
               r = e.debug_cluster_select(v, l, rp, count, k, m, largest);
             }
             py::dict d = exemplar_dict(r);
             d["tile"] = kExTile;
             d["chunk"] = kExChunk;
             return d;
           },
           py::arg("values"), py::arg("labels"), py::arg("rows") = py::none(), py::arg("k") = 1, py::arg("m") = 1,
           py::arg("largest") = false,
           "debug/test: the per-cluster selection kernels alone over host arrays (at most max_rows; k is the "
           "caller's); also the tile and chunk constants of the two passes")
      .def("silhouette", [](KMEngine& e, int slot, bool apply_filter, int scaler_mode,
                            std::optional<py::array_t<double, py::array::c_style | py::array::forcecast>> std,
                            bool per_row) {
        if (scaler_mode == kKmScalerGiven && (!std || std->size() != e.d()))
          throw std::invalid_argument("silhouette(): the given scaler needs d stds");
        KMSilResult r;
        {
          const double* sp = std ? std->data() : nullptr;
          py::gil_scoped_release nogil;
          r = e.silhouette(slot, apply_filter, scaler_mode, sp, per_row);
        }
        const KMScoreResult& b = r.batch;
        py::dict out;
        out["n_raw"] = b.n_raw;
        out["n_scored"] = b.n_scored;
        out["n"] = py::array_t<int64_t>(py::ssize_t(r.n.size()), r.n.data());
        out["s_fix"] = py::array_t<int64_t>(py::ssize_t(r.s_fix.size()), r.s_fix.data());
        out["n_single"] = r.n_single;
        out["n_undefined"] = r.n_undefined;
        out["nonempty"] = r.nonempty;
        out["cost"] = b.cost;
        out["sizes"] = py::array_t<int64_t>(py::ssize_t(b.sizes.size()), b.sizes.data());
        out["std"] = py::array_t<double>(py::ssize_t(b.std.size()), b.std.data());
        out["sil_ms"] = b.ms;
        if (r.per_row) {   // copies owned by the caller (the engine's pinned block is reused)
          const py::ssize_t n = r.rows ? py::ssize_t(b.n_scored) : 0;
          out["rows"] = py::array_t<int64_t>(n, r.rows);
          out["pred"] = py::array_t<int32_t>(n, r.labels);
          out["neighbor"] = py::array_t<int32_t>(n, r.neighbor);
          out["a"] = py::array_t<double>(n, r.a);
          out["b"] = py::array_t<double>(n, r.b);
          out["s"] = py::array_t<double>(n, r.s);
        }
        return out;
      }, py::arg("slot"), py::arg("apply_filter") = true, py::arg("scaler_mode") = 0, py::arg("std") = py::none(),
         py::arg("per_row") = false,
         "inference only: the silhouette words of the batch in `slot` under the current model (n[k], s_fix[k] = "
         "sum rint(s 2^36), n_single, n_undefined), with the batch's cost, sizes and std; per_row: also rows, "
         "pred, neighbor, a, b, s")
      .def_static("cost_shape", [](int dp) {
        const KmCostShape sh = km_cost_shape(dp);
        return py::make_tuple(sh.lanes_per_row, sh.rows_per_wave, sh.rows_per_wg);
      }, py::arg("dp"), "the cost kernel's (lanes per row, rows per wave, rows per workgroup) at padded width dp")
      .def_property_readonly("dp", &KMEngine::dp)
      .def("set_state", [](KMEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> c,
                           py::array_t<double, py::array::c_style | py::array::forcecast> w) {
        if (c.size() != py::ssize_t(e.k()) * e.d() || w.size() != e.k())
          throw std::invalid_argument("state shape mismatch");
        e.set_state(c.data(), w.data());
      })
      .def("get_state", [](const KMEngine& e) {
        py::array_t<double> c({py::ssize_t(e.k()), py::ssize_t(e.d())});
        py::array_t<double> w(py::ssize_t(e.k()));
        e.get_state(c.mutable_data(), w.mutable_data());
        return py::make_tuple(c, w);
      })
      .def("synchronize", &KMEngine::synchronize)
      .def("debug_labels", [](const KMEngine& e) {
        std::vector<int32_t> v;
        {
          py::gil_scoped_release nogil;
          v = e.debug_labels();
        }
        return py::array_t<int32_t>(py::ssize_t(v.size()), v.data());
      })
      .def("debug_features", [](const KMEngine& e) {
        std::vector<float> v;
        {
          py::gil_scoped_release nogil;
          v = e.debug_features();
        }
        const py::ssize_t dp = py::ssize_t(e.dp());
        py::array_t<float> a({py::ssize_t(v.size()) / dp, dp});
        std::copy(v.begin(), v.end(), a.mutable_data());
        return a;
      })
      .def_property_readonly("k", &KMEngine::k)
      .def_property_readonly("d", &KMEngine::d);
}

}  // namespace twtml
