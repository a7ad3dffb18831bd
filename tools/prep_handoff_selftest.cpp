// Sanitizer self-test of the LR engine's prepare-ahead handoff
// (csrc/hip/prep_handoff.h), with no GPU: a fake prep thread runs the worker
// side (next_job / packet_ready / job_done, with a settable "fail the n-th
// job" and a gate that holds a job open), the main thread plays process(),
// train()'s mid-loop gather and discard() with fake actions.  Built with
// -fsanitize=address,undefined and with -fsanitize=thread by
// tests/test_prep_handoff.py.  A deadlock ends in SIGALRM, not in a hang.
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hip/prep_handoff.h"

using twtml::PrepHandoff;
using Action = PrepHandoff::Action;
using BufState = PrepHandoff::BufState;
using Packet = PrepHandoff::Packet;

#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)

namespace {

constexpr int64_t kInlineMaxU = 7;   // pairs per rank of an all-gather issued in line by PrepareHere

struct Done {   // one finished job of the fake prep thread
  int slot;
  int64_t now_ms, max_u;
};

struct Rig {
  int64_t ready = 0;   // stands in for the mapped ready word
  PrepHandoff h;
  const bool dp;
  std::atomic<int> fail_job{0};   // the n-th job (1-based) fails before its packet
  std::atomic<bool> hold{false};  // jobs stay open while set
  std::mutex log_mu;
  std::vector<Done> log;
  int jobs = 0;
  std::thread worker;

  explicit Rig(bool dp_) : h(true, dp_, dp_ ? &ready : nullptr), dp(dp_), worker([this] { run(); }) {}
  ~Rig() {
    h.shutdown();
    worker.join();
  }
  static int64_t nu_of(int slot) { return 10 + slot; }
  int64_t ready_word() { return __atomic_load_n(&ready, __ATOMIC_ACQUIRE); }
  void run() {
    for (;;) {
      const PrepHandoff::Job j = h.next_job();
      if (j.buf < 0) return;
      std::exception_ptr err;
      try {
        if (++jobs == fail_job.load()) throw std::runtime_error("injected prep failure");
        int64_t max_u = -1;
        if (dp) {
          max_u = h.packet_ready(j.buf, nu_of(j.slot));
          if (max_u < 0) return;
        }
        while (hold.load()) std::this_thread::yield();
        std::lock_guard<std::mutex> lk(log_mu);
        log.push_back({j.slot, j.now_ms, max_u});
      } catch (...) {
        err = std::current_exception();
      }
      h.job_done(j.buf, err);
    }
  }
  std::vector<Done> done() {
    std::lock_guard<std::mutex> lk(log_mu);
    return log;
  }
  int find(int slot) {   // the buffer that holds `slot`, -1 if none
    for (int b = 0; b < 2; ++b)
      if (h.state(b) != BufState::Free && h.slot(b) == slot) return b;
    return -1;
  }
  int wait_state(int slot, BufState st) {
    int b;
    while ((b = find(slot)) < 0 || h.state(b) != st) std::this_thread::yield();
    return b;
  }
  // process() up to the training: the claim loop with fake actions.
  struct Played {
    PrepHandoff::Claim c;
    int gathers = 0, reports = 0;
  };
  Played play(int slot, int64_t now_ms, bool peer_fails = false) {
    Played p{h.claim(slot, now_ms)};
    for (; p.c.action != Action::Train && p.c.action != Action::PrepareHere; p.c = h.claim(slot, now_ms)) {
      if (p.c.action == Action::ReportLocalFailure) {
        ++p.reports;
      } else {
        CHECK(p.c.nu_local == nu_of(slot) && ready_word() == nu_of(slot) + 1);
        ++p.gathers;
        if (peer_fails) h.peer_failed(p.c.buf);
        else h.gathered(p.c.buf, nu_of(slot) + 100);
      }
    }
    if (p.c.action == Action::PrepareHere) {
      CHECK(h.state(p.c.buf) == BufState::Preparing && h.slot(p.c.buf) == slot && h.owns(slot));
      if (dp) h.gathered(p.c.buf, kInlineMaxU);
      h.prepared_here(p.c.buf);
    }
    CHECK(h.state(p.c.buf) == BufState::Ready && h.owns(slot));
    return p;
  }
  // slot 0 in line, then slot 1 goes to the prep thread: the common opening
  int open_with_two() {
    h.enqueue(0, 100);
    h.enqueue(1, 101);
    const Played p = play(0, 100);
    CHECK(p.c.action == Action::PrepareHere && !p.c.ahead);
    return p.c.buf;
  }
  bool all_free() { return h.state(0) == BufState::Free && h.state(1) == BufState::Free; }
};

template <class E, class F>
std::string thrown(F&& f) {   // what() of the E that f throws; "" if it does not
  try {
    f();
  } catch (const E& e) {
    return *e.what() ? e.what() : "?";
  }
  return "";
}

void in_order() {
  Rig r(false);
  r.h.enqueue(0, 100);
  CHECK(r.h.owns(0) && !r.h.owns(1));
  r.h.enqueue(1, 101);
  const auto p0 = r.play(0, 100);
  CHECK(p0.c.action == Action::PrepareHere && !p0.c.ahead);
  r.h.trained(p0.c.buf);
  CHECK(!r.h.owns(0) && r.h.owns(1));
  const auto p1 = r.play(1, 101);
  CHECK(p1.c.action == Action::Train && p1.c.ahead && p1.c.buf != p0.c.buf);
  const auto d = r.done();
  CHECK(d.size() == 1 && d[0].slot == 1 && d[0].now_ms == 101);
  r.h.trained(p1.c.buf);
  CHECK(r.all_free() && !r.h.owns(1));
}

void reprepare(bool fail_ahead, bool fail_here) {
  Rig r(false);
  if (fail_ahead) r.fail_job = 1;
  const int b0 = r.open_with_two();
  const int b1 = r.wait_state(1, BufState::Ready);
  r.h.trained(b0);
  const PrepHandoff::Claim c = r.h.claim(1, 999);   // another time than at enqueue
  CHECK(c.action == Action::PrepareHere && c.ahead && c.buf == b1);
  CHECK(r.h.state(b1) == BufState::Preparing && r.h.owns(1));
  if (!fail_here) {
    r.h.prepared_here(b1);
    CHECK(r.h.state(b1) == BufState::Ready);
    r.h.trained(b1);
    CHECK(r.all_free() && !r.h.owns(1));
    return;
  }
  // the re-prepare fails: the buffer must not stay "being prepared"
  r.h.release(b1);
  CHECK(r.all_free() && !r.h.owns(1));
  r.h.enqueue(1, 200);   // the slot number is used again
  const auto p = r.play(1, 200);   // returns (at the parent of this change it waited for ever)
  CHECK(p.c.action == Action::PrepareHere && !p.c.ahead);
  r.h.trained(p.c.buf);
  CHECK(r.all_free());
}

void failed_ahead_same_time() {
  Rig r(false);
  r.fail_job = 1;
  const int b0 = r.open_with_two();
  r.wait_state(1, BufState::Ready);
  r.h.trained(b0);
  CHECK(thrown<std::runtime_error>([&] { r.h.claim(1, 101); }).find("injected") != std::string::npos);
  CHECK(r.all_free() && !r.h.owns(1));
  // rethrown once: the next claim of the slot starts afresh
  r.h.enqueue(1, 101);
  const auto p = r.play(1, 101);
  CHECK(p.c.action == Action::PrepareHere && !p.c.ahead);
  r.h.trained(p.c.buf);
}

void eviction() {
  Rig r(false);
  const int b0 = r.open_with_two();
  r.h.enqueue(2, 102);
  r.wait_state(1, BufState::Ready);
  r.h.trained(b0);   // slot 2 goes to the prep thread
  r.wait_state(2, BufState::Ready);
  r.h.enqueue(3, 103);
  r.h.enqueue(4, 104);
  const int victim = r.h.slot(0);
  const auto p3 = r.play(3, 103);   // both buffers Ready with other batches: evicts buffer 0
  CHECK(p3.c.action == Action::PrepareHere && !p3.c.ahead && p3.c.buf == 0);
  CHECK(r.h.owns(victim) && r.find(victim) < 0);   // back in the queue ...
  r.h.trained(p3.c.buf);
  r.wait_state(victim, BufState::Ready);   // ... at its front: prepared before slot 4
  CHECK(r.find(4) < 0 && r.h.owns(4));
  const auto d = r.done();
  CHECK(d.size() == 3 && d[2].slot == victim && d[2].now_ms == 100 + victim);
  const auto pv = r.play(victim, 100 + victim);
  CHECK(pv.c.action == Action::Train && pv.c.ahead);
  r.h.trained(pv.c.buf);
}

void discards() {
  Rig r(false);
  r.h.enqueue(5, 105);   // queued
  r.h.discard(5);
  CHECK(!r.h.owns(5) && r.all_free());
  r.hold = true;         // being prepared: discard waits for the job
  const int b0 = r.open_with_two();
  r.wait_state(1, BufState::Preparing);
  std::thread opener([&] {
    for (int i = 0; i < 1000; ++i) std::this_thread::yield();
    r.hold = false;
  });
  r.h.discard(1);
  CHECK(r.done().size() == 1 && !r.h.owns(1) && r.find(1) < 0);
  opener.join();
  r.h.trained(b0);
  r.h.enqueue(2, 102);   // Ready
  r.h.enqueue(3, 103);
  const auto p2 = r.play(2, 102);
  r.wait_state(3, BufState::Ready);
  r.h.discard(3);
  CHECK(!r.h.owns(3) && r.find(3) < 0);
  r.h.trained(p2.c.buf);
  CHECK(r.all_free());
}

void owns_through_the_states() {
  Rig r(false);
  r.hold = true;
  const int b0 = r.open_with_two();
  const int b1 = r.wait_state(1, BufState::Preparing);
  CHECK(r.h.owns(1));
  r.hold = false;
  r.wait_state(1, BufState::Ready);
  CHECK(r.h.owns(1));
  r.h.trained(b0);
  CHECK(!r.h.owns(0));
  const auto p = r.play(1, 101);
  CHECK(p.c.action == Action::Train && p.c.buf == b1);
  r.h.trained(b1);
  CHECK(!r.h.owns(1) && r.all_free());
}

void dp_mid_loop_gather() {
  Rig r(true);
  const int b0 = r.open_with_two();
  PrepHandoff::Waiting w;  // the GD loop finds the next batch's packet
  while ((w = r.h.packet_waiting(b0)).buf < 0) std::this_thread::yield();
  CHECK(w.buf != b0 && w.nu_local == Rig::nu_of(1) && r.ready_word() == Rig::nu_of(1) + 1);
  CHECK(r.h.packet(w.buf) == Packet::Ready && r.h.state(w.buf) == BufState::Preparing);
  r.h.gathered(w.buf, 33);
  CHECK(r.ready_word() == 0 && r.h.packet_waiting(b0).buf < 0);
  r.h.trained(b0);
  const auto p = r.play(1, 101);
  CHECK(p.c.action == Action::Train && p.c.ahead && p.gathers == 0 && p.c.buf == w.buf);
  const auto d = r.done();
  CHECK(d.size() == 1 && d[0].max_u == 33);
  r.h.trained(p.c.buf);
  CHECK(r.all_free() && r.h.packet(0) == Packet::None && r.h.packet(1) == Packet::None);
}

void dp_inline_gather(bool peer_fails) {
  Rig r(true);
  const int b0 = r.open_with_two();
  r.h.trained(b0);
  if (peer_fails) {
    const std::string what = thrown<std::runtime_error>([&] { r.play(1, 101, true); });
    CHECK(what.find("peer rank failed") != std::string::npos);
    CHECK(r.all_free() && !r.h.owns(1) && r.done().empty());
    return;
  }
  const auto p = r.play(1, 101);
  CHECK(p.c.action == Action::Train && p.c.ahead && p.gathers == 1 && p.reports == 0);
  CHECK(r.ready_word() == 0 && r.h.packet(p.c.buf) == Packet::Gathered);
  const auto d = r.done();
  CHECK(d.size() == 1 && d[0].max_u == Rig::nu_of(1) + 100);
  r.h.trained(p.c.buf);
}

void dp_local_failure() {
  Rig r(true);
  r.fail_job = 1;
  const int b0 = r.open_with_two();
  r.h.trained(b0);
  int reports = 0;
  const std::string what = thrown<std::runtime_error>([&] {
    for (;;) {
      const PrepHandoff::Claim c = r.h.claim(1, 101);
      CHECK(c.action == Action::ReportLocalFailure);
      ++reports;
    }
  });
  CHECK(reports == 1 && what.find("injected") != std::string::npos);
  CHECK(r.all_free() && !r.h.owns(1) && r.ready_word() == 0);
}

void dp_order_is_enforced() {
  Rig r(true);
  r.open_with_two();   // slot 0 Ready (training), slot 1 with the prep thread
  r.h.enqueue(2, 102);
  CHECK(thrown<std::logic_error>([&] { r.h.claim(2, 102); }).find("submission order") != std::string::npos);
  CHECK(thrown<std::logic_error>([&] { r.h.discard(1); }).find("must be processed") != std::string::npos);
  CHECK(r.h.owns(1));
}

void shutdowns() {
  { Rig r(true); }   // the worker waits in next_job (maybe: it may not have got there yet)
  {
    Rig r(false);
    r.h.enqueue(0, 100);   // enqueue alone starts nothing
    for (int i = 0; i < 100; ++i) std::this_thread::yield();
    CHECK(r.all_free() && r.done().empty());
  }
  {
    Rig r(true);   // the worker waits in packet_ready
    const int b0 = r.open_with_two();
    while (r.h.packet_waiting(b0).buf < 0) std::this_thread::yield();
  }
}

}  // namespace

int main() {
  alarm(60);
  in_order();
  reprepare(false, false);                     // re-prepare, success
  reprepare(false, true);                      // re-prepare, failure
  failed_ahead_same_time();
  reprepare(true, false);                      // failed ahead, other time
  eviction();
  discards();
  owns_through_the_states();
  dp_mid_loop_gather();
  dp_inline_gather(false);
  dp_inline_gather(true);                      // peer failure
  dp_local_failure();
  dp_order_is_enforced();
  shutdowns();
  std::puts("prep handoff selftest ok");
  return 0;
}
