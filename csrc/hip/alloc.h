// Device allocations of the engines.  TWTML_POISON=<byte> fills every new
// buffer with that byte (debugging: a result that changes under poison reads
// memory it never wrote).  The owners that release them are in owned.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "common.h"

namespace twtml {

// Bytes the engines have allocated so far (monotonic): the difference across
// an engine's construction is its device footprint (HBM batch sizing).
inline std::atomic<uint64_t>& dev_alloc_bytes() {
  static std::atomic<uint64_t> total{0};
  return total;
}

// Bytes of dev_alloc buffers not released yet (DevArena, owned.h): back at
// its earlier value once the engines built since are gone.
inline std::atomic<uint64_t>& dev_live_bytes() {
  static std::atomic<uint64_t> live{0};
  return live;
}

// Bytes dev_alloc reserves for a request (what both counters move by).
inline size_t dev_alloc_size(size_t bytes) { return std::max<size_t>(1, bytes); }

inline void* dev_alloc(size_t bytes) {
  void* p = nullptr;
  bytes = dev_alloc_size(bytes);
  const hipError_t hipMalloc_status = hipMalloc(&p, bytes);
  if (hipMalloc_status != hipSuccess) (void)hipGetLastError();   // a refused allocation must not colour a later check
  TWTML_HIP_CHECK(hipMalloc_status);
  dev_alloc_bytes() += bytes;
  dev_live_bytes() += bytes;
  static const int poison = [] {
    const char* e = std::getenv("TWTML_POISON");
    return e && *e ? std::atoi(e) & 0xFF : -1;
  }();
  if (poison >= 0) {
    TWTML_HIP_CHECK(hipMemset(p, poison, bytes));
    TWTML_HIP_CHECK(hipDeviceSynchronize());
  }
  return p;
}

}  // namespace twtml
