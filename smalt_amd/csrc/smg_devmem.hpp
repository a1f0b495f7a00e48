// smg_devmem.hpp -- device memory and events with an owner, and the check of a HIP call, for the host side of the text parsers and
// of the index construction (smg_fasta.hip, smg_fastq_ref.hip, smg_reads_dev.hip, smg_indexbuild.hip).  An allocation or an event
// goes with the scope that holds it, on every return; what outlives the function is moved out (FastaParsed, BuiltIndex) or
// released to whoever records it.  The mapper's DevBuf<T> (smg_mapper.hpp) reports through the C ABI's error channel instead.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <utility>
#include <hip/hip_runtime.h>

namespace smg {

template <class T> class DevMem {        // n counts elements of T; move-only
 public:
  DevMem() = default;
  DevMem(DevMem &&o) noexcept { swap(o); }
  DevMem &operator=(DevMem &&o) noexcept { swap(o); return *this; }          // what this one held goes with o
  ~DevMem() { (void)reset(); }
  hipError_t alloc(size_t n) {                     // exactly n; what was held is freed
    (void)reset();
    const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
    if (e == hipSuccess) bytes_ = n * sizeof(T); else p_ = nullptr;
    return e;
  }
  hipError_t need(size_t n) {                      // at least n: an allocation that only grows, with a quarter of headroom
    const size_t b = n * sizeof(T);
    return b <= bytes_ && p_ ? hipSuccess : alloc((b + b / 4 + 256 + sizeof(T) - 1) / sizeof(T));
  }
  hipError_t reset() {
    const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
    p_ = nullptr; bytes_ = 0;
    return e;
  }
  T *release() { bytes_ = 0; return std::exchange(p_, nullptr); }           // the pointer is the caller's from here on
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t bytes() const { return bytes_; }

 private:
  void swap(DevMem &o) { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); }
  T *p_ = nullptr;
  size_t bytes_ = 0;
};

class DevEvent {                         // move-only
 public:
  DevEvent() = default;
  DevEvent(DevEvent &&o) noexcept { std::swap(e_, o.e_); }
  DevEvent &operator=(DevEvent &&o) noexcept { std::swap(e_, o.e_); return *this; }
  ~DevEvent() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create() { return hipEventCreate(&e_); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// "<the call>: <what HIP says about it>"
inline void hip_error_text(char *buf, size_t n, const char *call, hipError_t e) { snprintf(buf, n, "%s: %s", call, hipGetErrorString(e)); }

// in a function that reports through `err` / `errlen` and returns -1: owners free what was allocated so far
#define SMG_HIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { smg::hip_error_text(err, errlen, #x, e_); return -1; } } while (0)

}  // namespace smg
