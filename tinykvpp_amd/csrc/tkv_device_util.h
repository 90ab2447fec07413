// Host-side launch and scratch plumbing shared by the .hip files: the HIP error return, grid
// arithmetic, growing device arrays and the per-device scratch slot.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_engine.h"

// Returns TKV_IO_ERROR with HIP's text as tkv_last_error() when `call` fails.
#define TKV_HIP_RC(call)                                                         \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) return set_error(TKV_IO_ERROR, hipGetErrorString(e_)); \
  } while (0)

namespace tkv {

inline unsigned blocks(std::uint64_t n, std::uint64_t t) { return static_cast<unsigned>((n + t - 1) / t); }

// Workgroups of `waves` waves for nblocks items taken 64 per wave step: one per CU (at most cap), or
// fewer when the steps run out, and at least one. The launch then has wave_grid(...) * waves waves.
inline unsigned wave_grid(std::uint64_t nblocks, unsigned ncu, unsigned waves, unsigned cap = ~0u) {
  const std::uint64_t steps = (nblocks + 63u) / 64u;
  return static_cast<unsigned>(
      std::max<std::uint64_t>(1, std::min<std::uint64_t>(std::min(ncu, cap), (steps + waves - 1) / waves)));
}

// *p holds at least `want` units of `unit` bytes afterwards: grown by doubling, contents dropped.
inline int grow(void** p, std::uint64_t* cap, std::uint64_t want, std::uint64_t unit) {
  if (want <= *cap) return TKV_OK;
  const std::uint64_t c = std::max<std::uint64_t>(want, 2 * *cap);
  TKV_HIP_RC(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  TKV_HIP_RC(hipMalloc(p, c * unit));
  *cap = c;
  return TKV_OK;
}

// The calling thread's device's T, created on first use and kept for the process's lifetime. T's own
// one-time initialisation stays with the caller, under T's own mutex.
template <class T>
int per_device(T** out) {
  static std::mutex mu;
  static T* slot[64] = {};
  int dev = 0;
  TKV_HIP_RC(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return set_error(TKV_INVALID_ARGUMENT, "device index out of range");
  std::lock_guard<std::mutex> lk(mu);
  if (!slot[dev]) slot[dev] = new T();
  *out = slot[dev];
  return TKV_OK;
}

}  // namespace tkv
