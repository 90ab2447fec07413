// Host-side launch and scratch plumbing shared by the .hip files: the HIP error return, grid
// arithmetic, growing device arrays, the per-device scratch slot and its base (pinned result block,
// device words, the wait for a tagged result), the phase clock and the per-path stats of the
// tkv_debug_*_last / tkv_debug_*_phases hooks, and the scratch take that reports TKV_OUT_OF_MEMORY.
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

// A device array that grows by doubling and is freed with its owner.
struct DeviceBuf {
  void* p = nullptr;
  std::uint64_t cap = 0;  // in units of the T it was last taken as
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { (void)hipFree(p); }
  // At least `want` T (contents dropped when it grows); a failed allocation returns grow's code.
  template <class T>
  int take(std::uint64_t want, T** out) {
    if (int rc = grow(&p, &cap, want, sizeof(T))) return rc;
    *out = static_cast<T*>(p);
    return TKV_OK;
  }
};

// What every per-device scratch struct starts with (the DeviceBuf members are the deriving struct's):
// the lock of a call in progress, the pinned block a publish kernel writes results and a tag to, and a
// few device words (flags, counters) under the name the deriving struct gives them.
struct ScratchBase {
  std::mutex mu;
  int ncu = 0;
  std::uint64_t* h_res = nullptr;       // pinned, host_words words
  std::uint64_t* d_hres = nullptr;      // device view of h_res
  unsigned long long* words = nullptr;  // dev_words device words
  bool ready = false;
  ScratchBase() = default;
  ScratchBase(const ScratchBase&) = delete;
  ScratchBase& operator=(const ScratchBase&) = delete;
  ~ScratchBase() {
    (void)hipFree(words);
    (void)hipHostFree(h_res);
  }
  // Under mu, before every use: allocates what is still missing, so a call that failed half way leaks
  // nothing and the next one completes it. need_cus: a device that reports no compute unit is an error
  // (else the caller clamps ncu).
  int init(std::uint64_t host_words, std::uint64_t dev_words, bool need_cus) {
    if (ready) return TKV_OK;
    ncu = device_cu_count();
    if (need_cus && ncu <= 0) return set_error(TKV_IO_ERROR, "no device");
    if (!h_res) TKV_HIP_RC(hipHostMalloc(reinterpret_cast<void**>(&h_res), host_words * sizeof(std::uint64_t), hipHostMallocDefault));
    if (!d_hres) TKV_HIP_RC(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_hres), h_res, 0));
    if (!words) TKV_HIP_RC(hipMalloc(reinterpret_cast<void**>(&words), dev_words * sizeof(unsigned long long)));
    ready = true;
    return TKV_OK;
  }
  // After the launches up to a publish kernel: their launch errors, the stream's end, and the tag the
  // publish kernel left in h_res[idx] (anything else: `msg` as TKV_IO_ERROR).
  int wait(hipStream_t st, int idx, std::uint64_t tag, const char* msg) const {
    TKV_HIP_RC(hipGetLastError());
    TKV_HIP_RC(hipStreamSynchronize(st));
    if (h_res[idx] != tag) return set_error(TKV_IO_ERROR, msg);
    return TKV_OK;
  }
};

// Device events at the five boundaries of a call's four phases while `enable` is set; finish() leaves
// the phase times in ms[4] (zeros when disabled or an event failed).
struct PhaseClock {
  hipEvent_t e[5] = {};
  bool on = false;
  hipStream_t st;
  double* ms;
  PhaseClock(hipStream_t s, bool enable, double* out_ms) : st(s), ms(out_ms) {
    if (!enable) return;
    on = true;
    for (auto& x : e) on = on && hipEventCreate(&x) == hipSuccess;
  }
  PhaseClock(const PhaseClock&) = delete;
  PhaseClock& operator=(const PhaseClock&) = delete;
  void mark(int k) {
    if (on) (void)hipEventRecord(e[k], st);
  }
  void finish() {  // after the stream has been synchronised
    for (int k = 0; k < 4; ++k) {
      float t = 0;
      ms[k] = on && hipEventElapsedTime(&t, e[k], e[k + 1]) == hipSuccess ? t : 0.0;
    }
  }
  ~PhaseClock() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// What a path's tkv_debug_*_last and tkv_debug_*_phases hooks report for the calling thread; each
// path's .hip file keeps one thread_local instance. last[4]: what the thread's last device call did;
// phase[4]: its phase times, device events at the phase boundaries while timing is set; taken: the
// scratch bytes the call in progress has asked for (take below).
struct PathStats {
  std::uint64_t last[4] = {0, 0, 0, 0};
  int timing = 0;
  double phase[4] = {0, 0, 0, 0};
  std::uint64_t taken = 0;
  void begin() {  // a device call starts
    for (auto& v : last) v = 0;
    for (auto& v : phase) v = 0;
    taken = 0;
  }
  void get_last(std::uint64_t out[4]) const {
    for (int i = 0; i < 4; ++i) out[i] = last[i];
  }
  // Sets timing, copies the last call's phase times to out_ms (nullable); returns the earlier setting.
  int phases(int enable, double* out_ms) {
    const int prev = timing;
    timing = enable ? 1 : 0;
    if (out_ms)
      for (int i = 0; i < 4; ++i) out_ms[i] = phase[i];
    return prev;
  }
};

// b.take for a path whose failed scratch allocation is the caller's TKV_OUT_OF_MEMORY with the path's
// own text `msg`; the bytes asked for are added to `bytes`.
template <class T>
int take(DeviceBuf& b, std::uint64_t want, T** out, std::uint64_t& bytes, const char* msg) {
  if (b.take(want, out) != TKV_OK) return set_error(TKV_OUT_OF_MEMORY, msg);
  bytes += want * sizeof(T);
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

// The same for a T that derives from ScratchBase, initialised (ScratchBase::init).
template <class T>
int per_device_scratch(T** out, std::uint64_t host_words, std::uint64_t dev_words, bool need_cus) {
  T* sp = nullptr;
  if (int rc = per_device(&sp)) return rc;
  std::lock_guard<std::mutex> lk(sp->mu);
  if (int rc = sp->init(host_words, dev_words, need_cus)) return rc;
  *out = sp;
  return TKV_OK;
}

}  // namespace tkv
