// Streaming k-means engine (K8-K11) on one GPU, RCCL data parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <memory>
#include <vector>

#include "comm.h"
#include "common.h"
#include "engine.h"
#include "exemplars.h"
#include "kernels.h"
#include "owned.h"

namespace twtml {

struct KMConfig {
  int32_t k = 3;
  int32_t text_dims = 0;       // hashed bigram dims appended to [retweetCount, followers]
  double decay = 0.8705505632961241;  // setHalfLife(5, "batches")
  int32_t points_unit = 0;     // timeUnit "points"
  int32_t scale = 1;           // StandardScaler(false, true) per batch
  // matrix-core assignment: 1 = bf16x3 split MFMA where 16 <= dp <= 128 and
  // k <= 4096 (fp32 MFMA otherwise), 2 = fp32 MFMA only, 0 = scalar fp32
  int32_t mfma = 1;
  int64_t max_rows = 1 << 16;
  int64_t max_units = (1 << 16) * 281;
  int32_t force_dp = 0;        // DP collectives even with a world-1 communicator (also TWTML_FORCE_DP=1)
  int32_t raw_slots = kDefaultRawSlots;   // device raw-batch slots (H2D run-ahead depth + 1)
};

struct KMResult {
  int64_t n_raw = 0, n_local = 0, n_global = 0;
  std::vector<double> std;     // scaler std per column
  std::vector<int32_t> labels; // labels of this rank's points (new model) if requested
  float ms = 0.f;
};

// score(): how the scaler factors are chosen
constexpr int kKmScalerBatch = 0;   // StandardScaler fitted on the scored rows (as training, no collective)
constexpr int kKmScalerGiven = 1;   // the caller's std[d]: factor_j = std_j != 0 ? 1 / std_j : 0
constexpr int kKmScalerNone = 2;    // factor 1

// The arrays point into the engine's pinned buffer: valid until the next score().
struct KMScoreResult {
  int64_t n_raw = 0, n_scored = 0;
  const int64_t* rows = nullptr;    // [n_scored] raw row ids, ascending
  const int32_t* labels = nullptr;  // [n_scored] closest centre
  const double* dist2 = nullptr;    // [n_scored] squared distance to it, in the scaled space
  double cost = 0.0;                // sum of dist2 (KMeansModel.computeCost), summed on the device
  std::vector<int64_t> sizes;       // [k] rows per cluster
  std::vector<double> std;          // [d] column stds used (empty: no scaler)
  float ms = 0.f;                   // device time of the kernels (events)
};

// top(): score()'s batch-wide outputs and the n best rows by squared distance
// (top.payload: their labels).  top's arrays point into the engine's pinned
// block: valid until the next top().
struct KMTopResult {
  KMScoreResult batch;   // n_raw, n_scored, cost, sizes, std, ms (through the selection); no per-row arrays
  TopResult top;
};

// silhouette(): the batch's integer words (models/silhouette.py), score()'s
// batch-wide outputs, and with per_row the row arrays, which point into the
// engine's pinned block: valid until the next silhouette().
struct KMSilResult {
  KMScoreResult batch;              // n_raw, n_scored, cost, sizes, std, ms (the whole pass); no per-row arrays
  std::vector<int64_t> n, s_fix;    // [k] rows with a defined s | sum rint(s 2^36), per own cluster
  int64_t n_single = 0, n_undefined = 0, nonempty = 0;
  bool per_row = false;
  const int64_t* rows = nullptr;    // [n_scored] raw row ids, ascending
  const int32_t* labels = nullptr;  // [n_scored] own cluster (score()'s labels)
  const int32_t* neighbor = nullptr;  // [n_scored] closest other cluster by mean distance, -1: none
  const double *a = nullptr, *b = nullptr, *s = nullptr;
};

// exemplars(): score()'s batch-wide outputs and, per cluster, the m rows
// nearest their centre (largest: farthest), models/exemplars.py.  The arrays
// point into the engine's pinned block: valid until the next exemplars() or
// debug_cluster_select().
struct KMExemplarResult {
  KMScoreResult batch;              // n_raw, n_scored, cost, sizes, std, ms (through the selection); no per-row arrays
  int32_t k = 0, m = 0;
  int64_t n_nan = 0;
  const int64_t* counts = nullptr;  // [k] entries selected
  const int64_t* bits = nullptr;    // [k][m] value bits, best first; 0 beyond counts[c]
  const int64_t* rows = nullptr;    // [k][m] raw row ids; -1 beyond counts[c]
  float ex_ms = 0.f;                // device time (events): exemplars() the whole pass, debug: the selection
  float sel_ms = 0.f;               // ... of the selection kernels alone
};

class KMEngine {
 public:
  KMEngine(int device, const KMConfig& cfg, std::shared_ptr<Comm> comm);
  ~KMEngine();
  void submit(const HostBatch& hb, int64_t n, int64_t bytes, int slot, const uint8_t* ext_text = nullptr);
  KMResult process(int slot, bool want_labels);
  // Inference only: clusters and cost of the batch in `slot` under the current
  // model.  Filter (apply_filter: the training filter, else every row),
  // features, scaler factors by `scaler_mode` (std: kKmScalerGiven's d
  // values), the training assignment with its fp64 near-tie refine, then the
  // fp64 cost pass.  Leaves the model, the other raw slots and the
  // communicator untouched; reuses the batch scratch of process() (both end in
  // a stream sync, so they never overlap).
  KMScoreResult score(int slot, bool apply_filter, int scaler_mode, const double* std);
  // The n rows (1 <= n <= kTopNMax) farthest from their centres (largest; else
  // the closest): score() up to and including the cost pass, then the
  // selection of topn.hip over the squared distances with the kept row ids
  // and the labels as payload.  Only the result block, the cost, the sizes and
  // the stds leave the device; no communicator is called.
  KMTopResult top(int slot, bool apply_filter, int scaler_mode, const double* std, int n, bool largest);
  // The silhouette of the current model on the batch in `slot` (MLlib's
  // ClusteringEvaluator, squared Euclidean; models/silhouette.py): score() up
  // to and including the cost pass, the batch's own cluster means by the
  // training path's exact integer sums, dev2 by the cost kernel against them,
  // W by an order-independent fixed-point sum, then the neighbour pass of
  // silhouette.hip.  Only 2k + 4 words, the cost, the sizes and the stds leave
  // the device (per_row: also the row arrays).  score()'s guarantees: no
  // communicator call, the model and its cached centres untouched; the
  // scratch is allocated by the first call.
  KMSilResult silhouette(int slot, bool apply_filter, int scaler_mode, const double* std, bool per_row);
  // Per cluster, the m rows (1 <= m <= kExMaxM, k m <= kExMaxCells) nearest
  // their centre (largest: farthest from it): score() up to and including the
  // cost pass, then the segmented selection of exemplars.hip over the squared
  // distances, the labels and the kept row ids, with the cost pass's cluster
  // sizes as the candidates' exact capacity.  Only the result block, the cost,
  // the sizes and the stds leave the device.  score()'s guarantees: no
  // communicator call; the model, its cached centres, the other raw slots and
  // a pending update untouched; the scratch is allocated by the first call.
  KMExemplarResult exemplars(int slot, bool apply_filter, int scaler_mode, const double* std, int m, bool largest);
  // Debug/test: the selection kernels alone on the caller's arrays (count <=
  // max_rows; rows may be null); k is independent of the model's.  The arrays
  // take the place of a scoring pass's outputs, so debug_labels() and the
  // pinned arrays of the last score() are overwritten.
  KMExemplarResult debug_cluster_select(const double* values, const int32_t* labels, const int64_t* rows,
                                        int64_t count, int k, int m, bool largest);
  // Forget a submitted batch that will not be processed: waits for its H2D
  // (the staging buffer may then be rewritten); the copy stream keeps the
  // slot's next H2D in order behind it.
  void discard(int slot) { raw_.wait_h2d(slot); }
  void set_state(const double* centers, const double* weights);
  void get_state(double* centers, double* weights) const;
  // Debug/test: the labels left by the last process() (the update's
  // assignment with the old centres when want_labels was false) or score(),
  // whichever ran last.
  std::vector<int32_t> debug_labels() const;
  // Debug/test: the unscaled fp32 feature rows [n_local][dp] of the last
  // batch, processed or scored.
  std::vector<float> debug_features() const;
  int k() const { return cfg_.k; }
  int d() const { return d_; }
  int dp() const { return dp_; }
  int64_t h2d_bytes() const { return raw_.h2d_bytes(); }
  int raw_slots() const { return raw_.count(); }
  void synchronize();

 private:
  // Exact integer column moments of X_ (kmeans.hip K11) on the host: qmom_ ->
  // host_q_, the kept-row count -> host_out_ + 1; syncs `s`.
  void fit_moments(bool reduce, hipStream_t s);
  // Host factors -> fac64_ / fac32_ by scaler mode (batch: from host_q_ and
  // the n rows fitted); `std` receives the d stds used (none: empty).
  void upload_factors(int mode, int64_t n, const double* given, std::vector<double>& std, hipStream_t s);
  void ensure_score();
  void ensure_top();
  void ensure_sil();
  void ensure_ex(int64_t kcap, size_t out_words);
  // The result block of a selection of (k, m) and, with `cost`, the cost and
  // the engine's sizes, copied to ex_host_ (syncs the compute stream).
  KMExemplarResult ex_result(int k, int m, const double* cost);
  // What score() and top() share: filter .. the cost pass of the batch in
  // `slot`, ev0_ recorded first.  Returns the scored rows n (res.n_raw,
  // n_scored, sizes and std filled) and the device cost word; n == 0: nothing
  // was assigned, ev1_ is recorded and the stream synchronised.
  int64_t score_kernels(const char* who, int slot, bool apply_filter, int scaler_mode, const double* std,
                        KMScoreResult& res, double** cost);
  int device_;
  KMConfig cfg_;
  int d_, dp_;
  bool dist_ = false;   // DP collectives: world > 1, or forced with a world-1 communicator
  std::shared_ptr<Comm> comm_;
  // Members are destroyed in reverse order: the streams outlive every
  // buffer, event and raw slot declared below them.
  Stream compute_, copy_;
  DevArena arena_;                     // owns every device buffer below (prep_'s included)
  RawSlots raw_;
  DevPrepared prep_{};
  float* X_ = nullptr;
  double *centers_ = nullptr, *weights_ = nullptr, *sums_ = nullptr;
  int64_t* sums_i_ = nullptr;          // [k d + k] per-cluster integer sums of q, counts (all-reduced)
  int64_t* qmom_ = nullptr;            // [d] column max | n | [d][4] integer moments (all-reduced)
  Pinned<int64_t> host_q_;             // pinned copy of qmom_
  Pinned<void> host_fac_;              // pinned [dp] fp64 + [dp] fp32 factors (H2D staging)
  float *c32_ = nullptr, *cnorm_ = nullptr, *fac32_ = nullptr;
  double *fac64_ = nullptr, *blend_ = nullptr;
  int32_t *labels_ = nullptr, *order_ = nullptr, *refine_ = nullptr;
  uint16_t* frag_ = nullptr;           // bf16x3 centre fragments
  float* cnp_ = nullptr;               // |c|^2 padded to 32-centre tiles
  int64_t* lhist_ = nullptr;
  uint8_t* lower_page_ = nullptr;
  uint16_t* lower_blocks_ = nullptr;
  Pinned<double> host_out_;
  Event ev0_, ev1_;
  // score() only, allocated by its first call
  double *dist2_ = nullptr, *cost_part_ = nullptr;   // [R] | [partials + 1]: the partials, then the cost
  size_t cost_parts_ = 0;
  Pinned<void> score_host_;            // [R] rows | [R] dist2 | cost | [k] sizes | [R] labels
  // top() only, allocated by its first call
  TopScratch top_sc_{};
  Pinned<int64_t> top_host_;           // result block of kTopNMax | cost | [k] sizes
  // exemplars() only, allocated by its first call (debug_cluster_select():
  // regrown for a larger k of the caller's)
  ExScratch ex_sc_{};
  int64_t* ex_buf_ = nullptr;          // the scratch ex_sc_ is carved from
  int64_t* ex_dbg_sizes_ = nullptr;    // debug_cluster_select(): [ex_dbg_k_] sizes of the caller's labels
  int ex_dbg_k_ = 0;
  Pinned<int64_t> ex_host_;            // result block | cost | [k] sizes
  size_t ex_host_words_ = 0;
  Event ex_ev_;                        // before the selection
  // silhouette() only, allocated by its first call
  double *sil_mean_ = nullptr, *sil_dev2_ = nullptr, *sil_part_ = nullptr;   // [k d] | [R] | [partials + 1]
  double *sil_W_ = nullptr, *sil_V_ = nullptr;                               // [k] each
  float *sil_mu32_ = nullptr, *sil_B_ = nullptr;                             // [k dp] | [k]
  unsigned long long* sil_wacc_ = nullptr;                                   // [k] max bits | [k] fixed-point sums
  int64_t *sil_hist_ = nullptr, *sil_sizes_ = nullptr, *sil_words_ = nullptr;   // [k + 1] | [k] | [2k + 4]
  int32_t* sil_nb_ = nullptr;                                                // [R]
  double *sil_a_ = nullptr, *sil_b_ = nullptr, *sil_s_ = nullptr;            // [R] each
  // words | cost | [k] sizes | [R] rows | [R] a | [R] b | [R] s | [R] labels | [R] neighbor
  Pinned<void> sil_host_;
};

void bind_kmeans(pybind11::module_& m);
// A selection's result as a dict of arrays owned by the caller (bindings.cpp).
pybind11::dict top_dict(const TopResult& r);
pybind11::dict exemplar_dict(const KMExemplarResult& r);

}  // namespace twtml
