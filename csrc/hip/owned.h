// Owners of the engines' GPU resources: each releases what it holds when it
// is destroyed, so an engine (or a constructor that throws half-way) frees
// its device buffers, pinned host buffers, events and streams through its
// members' destructors.  All are move-only.  Destructors ignore HIP errors:
// the engines report a device fault before their members go.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "alloc.h"

namespace twtml {

// Device buffers of one owner (an engine, a prepared buffer, a raw slot).
// The kernel-argument structs keep plain pointers into it.  No lock: an arena
// is used by one thread at a time.
class DevArena {
 public:
  DevArena() = default;
  DevArena(DevArena&&) noexcept = default;   // leaves the source empty; no assignment
  ~DevArena() { reset(); }

  template <typename T>
  T* alloc(size_t n) {
    bufs_.reserve(bufs_.size() + 1);   // the record below cannot throw
    T* p = static_cast<T*>(dev_alloc(n * sizeof(T)));
    bufs_.push_back({p, dev_alloc_size(n * sizeof(T))});
    return p;
  }
  // Release one buffer of this arena (null: nothing) and null the pointer.
  template <typename T>
  void free(T*& p) {
    for (size_t i = 0; p && i < bufs_.size(); ++i)
      if (bufs_[i].first == p) {
        release(bufs_[i]);
        bufs_.erase(bufs_.begin() + i);
        break;
      }
    p = nullptr;
  }
  // Replace p by a new buffer of n elements (contents are not kept).  A
  // regrowth is expensive: hipFree waits for the whole device, so whatever
  // else runs meanwhile (the batch in training, when the prep thread grows a
  // buffer) stalls -- the engines size their buffers for the configuration's
  // largest case up front and grow only beyond it.  `sync`: the stream whose
  // queued work may still use p, synchronised before a live p is freed; null
  // where the caller has synchronised already.
  template <typename T>
  T* grow(T*& p, size_t n, hipStream_t sync) {
    if (p && sync) TWTML_HIP_CHECK(hipStreamSynchronize(sync));
    free(p);
    return p = alloc<T>(n);
  }
  void reset() {
    for (auto it = bufs_.rbegin(); it != bufs_.rend(); ++it) release(*it);
    bufs_.clear();
  }

 private:
  static void release(const std::pair<const void*, size_t>& b) {
    (void)hipFree(const_cast<void*>(b.first));
    dev_live_bytes() -= b.second;
  }
  std::vector<std::pair<const void*, size_t>> bufs_;
};

// Page-locked host memory (hipHostMalloc); mapped buffers also carry their
// device address.  Converts to T* like the raw pointer it replaces.
template <typename T>
class Pinned {
 public:
  Pinned() = default;
  Pinned(Pinned&& o) noexcept : host_(std::exchange(o.host_, nullptr)), dev_(std::exchange(o.dev_, nullptr)) {}
  Pinned& operator=(Pinned&& o) noexcept { return std::swap(host_, o.host_), std::swap(dev_, o.dev_), *this; }
  ~Pinned() { reset(); }

  // (Re)allocate `bytes` with hipHostMalloc `flags`; the old buffer goes first.
  void alloc(size_t bytes, unsigned flags) {
    reset();
    TWTML_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host_), bytes, flags));
    if (flags & hipHostMallocMapped)
      TWTML_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_), host_, 0));
  }
  void reset() {
    if (host_) (void)hipHostFree(host_);
    host_ = dev_ = nullptr;
  }
  T* get() const { return host_; }
  T* dev() const { return dev_; }   // mapped buffers: the address kernels write to
  operator T*() const { return host_; }

 private:
  T* host_ = nullptr;
  T* dev_ = nullptr;
};

class Event {
 public:
  Event() = default;
  explicit Event(unsigned flags) { TWTML_HIP_CHECK(hipEventCreateWithFlags(&e_, flags)); }
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept { return std::swap(e_, o.e_), *this; }   // o's destructor releases the old one
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

class Stream {
 public:
  Stream() = default;
  explicit Stream(unsigned flags) { TWTML_HIP_CHECK(hipStreamCreateWithFlags(&s_, flags)); }
  Stream(unsigned flags, int priority) { TWTML_HIP_CHECK(hipStreamCreateWithPriority(&s_, flags, priority)); }
  // restricted to the CUs of `cu_mask` (bit i: CU i)
  explicit Stream(const std::vector<uint32_t>& cu_mask) {
    TWTML_HIP_CHECK(hipExtStreamCreateWithCUMask(&s_, uint32_t(cu_mask.size()), cu_mask.data()));
  }
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept { return std::swap(s_, o.s_), *this; }
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace twtml
