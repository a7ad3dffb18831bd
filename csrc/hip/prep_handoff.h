// Prepare-ahead handoff of LREngine's prepared-batch buffers (engine.h
// PrepBuf) between the training thread and the prep thread.  Host only: no
// HIP and no collective is called here.  Every function decides under the
// one lock what happens next and returns; the engine acts outside it and
// reports back what happened.  tools/prep_handoff_selftest.cpp drives it with
// fakes under the sanitizers.
//
// Buffers are named by index (the engine's pb_[buf]).  A buffer is Free,
// Preparing (the prep thread or the training thread works on it) or Ready
// (prepared, or failed with a stored error).  Under DP the prep thread's local
// part ends in a packet that the training thread all-gathers:
//   None -> Ready (announced; the mapped ready word holds nu_local + 1)
//        -> Gathered (ready word 0; the prep thread finishes the batch)
//         | PeerFailed (a peer reported a failed prep: no all-gather)
//   None -> FailureReported (this rank failed before its packet and has told
//           its peers, once)
// The batch's raw slot, time, packet size (nu_local) and the all-gather's
// pairs per rank (max_u) live here and nowhere else: the engine's prepare
// functions get them as arguments.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <iterator>
#include <mutex>
#include <stdexcept>
#include <utility>

namespace twtml {

class PrepHandoff {
 public:
  enum class BufState { Free, Preparing, Ready };
  enum class Packet { None, Ready, Gathered, PeerFailed, FailureReported };
  enum class Action { Train, GatherInline, ReportLocalFailure, PrepareHere };
  struct Job {      // buf < 0: shut down
    int buf = -1, slot = -1;
    int64_t now_ms = 0;
  };
  struct Claim {    // ahead: the batch was (being) prepared ahead; nu_local: GatherInline's packet
    Action action;
    int buf;
    bool ahead;
    int64_t nu_local;
  };
  struct Waiting {  // buf < 0: no packet waits
    int buf = -1;
    int64_t nu_local = 0;
  };

  // overlap: two buffers and a prep thread, else one buffer prepared in line.
  // ready_word: DP, the mapped word the GD kernels read (null otherwise).
  PrepHandoff(bool overlap, bool dp, int64_t* ready_word)
      : nbuf_(overlap ? 2 : 1), overlap_(overlap), dp_(dp), ready_(ready_word) {}

  // ---- submit side ----
  void enqueue(int slot, int64_t now_ms) {
    std::lock_guard<std::mutex> lk(mu_);
    queue_.push_back({slot, now_ms});
    cv_.notify_all();
  }
  // `slot` is in the prepare-ahead queue or in a buffer.
  bool owns(int slot) const {
    std::lock_guard<std::mutex> lk(mu_);
    for (const auto& q : queue_)
      if (q.first == slot) return true;
    return find_locked(slot) >= 0;
  }

  // ---- prep thread ----
  Job next_job() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return stop_ || job_ >= 0; });
    if (stop_) return {};
    return {job_, buf_[job_].slot, buf_[job_].now_ms};
  }
  // DP: announce the packet and wait for the training thread's all-gather.
  // Returns its pairs per rank, -1 on shutdown; throws if a peer failed.
  int64_t packet_ready(int buf, int64_t nu_local) {
    std::unique_lock<std::mutex> lk(mu_);
    Buf& b = buf_[buf];
    b.nu_local = nu_local;
    b.packet = Packet::Ready;
    __atomic_store_n(ready_, nu_local + 1, __ATOMIC_RELEASE);
    cv_.notify_all();
    cv_.wait(lk, [&] { return stop_ || b.packet != Packet::Ready; });
    if (stop_) return -1;
    if (b.packet == Packet::PeerFailed) throw std::runtime_error("DP: a peer rank failed to prepare this batch");
    return b.max_u;
  }
  void job_done(int buf, std::exception_ptr error) {
    std::lock_guard<std::mutex> lk(mu_);
    buf_[buf].error = error;
    buf_[buf].state = BufState::Ready;
    job_ = -1;
    cv_.notify_all();
  }
  void shutdown() {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
    cv_.notify_all();
  }

  // ---- training thread ----
  // What process() does next for the batch in `slot`; called again after
  // GatherInline and ReportLocalFailure.  A stored error is rethrown, once,
  // after the buffer is freed.
  Claim claim(int slot, int64_t now_ms) {
    std::unique_lock<std::mutex> lk(mu_);
    int k = find_locked(slot);
    if (k >= 0) {
      Buf& b = buf_[k];
      if (dp_) {
        // the packets were all-gathered during the previous batch, or are
        // now, in line -- the same choice on every rank (it follows the
        // all-reduced ready words); then the prep thread finishes the layout
        cv_.wait(lk, [&] { return b.packet != Packet::None || b.state == BufState::Ready; });
        if (b.packet == Packet::Ready) return {Action::GatherInline, k, true, b.nu_local};
        if (b.packet == Packet::None && b.error) {   // failed before its packet: tell the peers
          b.packet = Packet::FailureReported;
          return {Action::ReportLocalFailure, k, true, 0};
        }
      }
      cv_.wait(lk, [&] { return b.state == BufState::Ready; });
      // one GPU: prepared ahead with the batch time given at submit; a
      // different time here is re-prepared (a failure under the old time too)
      const bool retime = !dp_ && b.now_ms != now_ms;
      if (b.error && !retime) {
        std::exception_ptr err = b.error;
        free_locked(b);
        std::rethrow_exception(err);
      }
      if (retime) {
        take_locked(b, slot, now_ms);
        return {Action::PrepareHere, k, true, 0};
      }
      schedule_locked();   // batch t+1's prep overlaps batch t's training
      return {Action::Train, k, true, 0};
    }
    // not prepared ahead: drop it from the queue, prepare in line
    for (auto it = queue_.begin(); it != queue_.end(); ++it)
      if (it->first == slot) {
        queue_.erase(it);
        break;
      }
    // DP: every rank must issue the same collectives in the same order: a
    // batch prepared (and possibly all-gathered) ahead may not be skipped
    for (int i = 0; dp_ && i < nbuf_; ++i)
      if (buf_[i].state != BufState::Free)
        throw std::logic_error("DP: batches must be processed in submission order");
    for (int i = 0; i < nbuf_; ++i)
      if (buf_[i].state == BufState::Free) k = i;
    if (k < 0) {
      // one GPU: every buffer holds a batch prepared ahead that is not this
      // one (submitted but processed out of order): evict one -- its slot
      // goes back to the front of the queue and is prepared again when due
      cv_.wait(lk, [&] { return job_ < 0; });
      for (int i = 0; i < nbuf_ && k < 0; ++i)
        if (buf_[i].state == BufState::Ready) {
          queue_.push_front({buf_[i].slot, buf_[i].now_ms});
          free_locked(buf_[i]);
          k = i;
        }
      if (k < 0) throw std::logic_error("no free prepared-batch buffer");
    }
    take_locked(buf_[k], slot, now_ms);
    return {Action::PrepareHere, k, false, 0};
  }
  // PrepareHere succeeded (a failed one is release()d): the batch trains next.
  void prepared_here(int buf) {
    std::lock_guard<std::mutex> lk(mu_);
    buf_[buf].state = BufState::Ready;
    schedule_locked();
    cv_.notify_all();
  }
  // DP: the all-gather of buf's packet is issued, max_u pairs per rank.
  void gathered(int buf, int64_t max_u) {
    std::lock_guard<std::mutex> lk(mu_);
    buf_[buf].max_u = max_u;
    buf_[buf].packet = Packet::Gathered;
    __atomic_store_n(ready_, int64_t(0), __ATOMIC_RELEASE);
    cv_.notify_all();
  }
  // DP: a peer's prep failed, no all-gather: the prep thread raises.
  void peer_failed(int buf) {
    std::lock_guard<std::mutex> lk(mu_);
    buf_[buf].packet = Packet::PeerFailed;
    cv_.notify_all();
  }
  // DP, GD loop: the other buffer's announced packet, if any.
  Waiting packet_waiting(int training_buf) const {
    std::lock_guard<std::mutex> lk(mu_);
    Waiting w;
    for (int i = 0; i < nbuf_; ++i)
      if (i != training_buf && buf_[i].packet == Packet::Ready) w = {i, buf_[i].nu_local};
    return w;
  }
  // The batch in `buf` is trained: free it and prepare the next one ahead.
  void trained(int buf) {
    std::lock_guard<std::mutex> lk(mu_);
    free_locked(buf_[buf]);
    schedule_locked();
  }
  // Preparing here or training the batch in `buf` failed: free it.
  void release(int buf) {
    std::lock_guard<std::mutex> lk(mu_);
    free_locked(buf_[buf]);
  }
  // Forget a submitted batch (one GPU only): out of the queue, and out of a
  // buffer once its preparation has finished.
  void discard(int slot) {
    std::unique_lock<std::mutex> lk(mu_);
    if (dp_)   // every rank must issue the same collectives: no rank may skip a batch
      throw std::logic_error("DP: every submitted batch must be processed, in submission order");
    for (auto it = queue_.begin(); it != queue_.end();)
      it = it->first == slot ? queue_.erase(it) : std::next(it);
    for (int i = 0; i < nbuf_; ++i) {
      Buf& b = buf_[i];
      if (b.state == BufState::Free || b.slot != slot) continue;
      cv_.wait(lk, [&] { return b.state == BufState::Ready; });
      free_locked(b);
    }
    schedule_locked();
  }

  // the raw slot of the batch in `buf` (set when the buffer was taken)
  int slot(int buf) const {
    std::lock_guard<std::mutex> lk(mu_);
    return buf_[buf].slot;
  }
  BufState state(int buf) const {
    std::lock_guard<std::mutex> lk(mu_);
    return buf_[buf].state;
  }
  Packet packet(int buf) const {
    std::lock_guard<std::mutex> lk(mu_);
    return buf_[buf].packet;
  }

 private:
  struct Buf {
    BufState state = BufState::Free;
    Packet packet = Packet::None;
    int slot = -1;
    int64_t now_ms = 0;
    std::exception_ptr error;
    int64_t nu_local = 0;   // this rank's active ids (packet pairs)
    int64_t max_u = 0;      // pairs per rank in the all-gather
  };
  int find_locked(int slot) const {
    for (int i = 0; i < nbuf_; ++i)
      if (buf_[i].state != BufState::Free && buf_[i].slot == slot) return i;
    return -1;
  }
  // the one way a buffer is given back
  void free_locked(Buf& b) {
    b.state = BufState::Free;
    b.packet = Packet::None;
    b.error = nullptr;
  }
  void take_locked(Buf& b, int slot, int64_t now_ms) {
    b.state = BufState::Preparing;
    b.packet = Packet::None;
    b.error = nullptr;
    b.slot = slot;
    b.now_ms = now_ms;
  }
  // start preparing the next submitted slot if a buffer and the prep thread are free
  void schedule_locked() {
    if (!overlap_ || job_ >= 0 || queue_.empty()) return;
    int free_buf = -1;
    for (int i = 0; i < nbuf_; ++i)
      if (buf_[i].state == BufState::Free) free_buf = i;
    if (free_buf < 0) return;
    const auto next = queue_.front();
    if (find_locked(next.first) >= 0) return;   // already there
    queue_.pop_front();
    take_locked(buf_[free_buf], next.first, next.second);
    job_ = free_buf;
    cv_.notify_all();
  }

  const int nbuf_;
  const bool overlap_, dp_;
  int64_t* const ready_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<int, int64_t>> queue_;   // submitted (slot, now_ms), in order
  Buf buf_[2];
  int job_ = -1;        // the prep thread's buffer
  bool stop_ = false;
};

}  // namespace twtml
