// Move-only owners of the HIP resources of libzkp_amd: device buffers, pinned host buffers,
// streams and events.  Each is empty by default (classes construct their members before they
// select a device), creates its resource on the CURRENT device through HIPX, and releases it in
// its destructor; no owner ever calls hipSetDevice.  All convert implicitly to the raw pointer or
// handle, so launches, copies and event calls read as before.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

#include "hip_check.hpp"

namespace zkp {

namespace detail {

struct DevAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};

// `count` elements of T from allocator A (a zero count is the caller's business)
template <class T, class A>
class Buf {
 public:
  Buf() = default;
  explicit Buf(size_t count) : n_(count) { HIPX(A::alloc(reinterpret_cast<void**>(&p_), count * sizeof(T))); }
  ~Buf() { reset(); }
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  size_t count() const { return n_; }
  void reset() {
    if (p_) A::free(p_);
    p_ = nullptr;
    n_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace detail

template <class T = uint32_t>
using DevBuf = detail::Buf<T, detail::DevAlloc>;  // hipMalloc / hipFree
template <class T>
using PinnedBuf = detail::Buf<T, detail::PinnedAlloc>;  // hipHostMalloc / hipHostFree

namespace detail {

inline hipError_t drain_and_destroy(hipStream_t s) {
  (void)hipStreamSynchronize(s);
  return hipStreamDestroy(s);
}

// a stream or event handle H, released by Destroy
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  ~Handle() { reset(); }
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  H get() const { return h_; }
  operator H() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 protected:
  H h_ = nullptr;
};

}  // namespace detail

// A stream; the destructor drains it before destroying it.
struct Stream : detail::Handle<hipStream_t, detail::drain_and_destroy> {
  Stream() = default;
  explicit Stream(unsigned flags) { HIPX(hipStreamCreateWithFlags(&h_, flags)); }
  Stream(unsigned flags, int priority) { HIPX(hipStreamCreateWithPriority(&h_, flags, priority)); }
};

// An event: Event(true) with timing (hipEventElapsedTime), Event(false) hipEventDisableTiming.
struct Event : detail::Handle<hipEvent_t, hipEventDestroy> {
  Event() = default;
  explicit Event(bool timing) { HIPX(hipEventCreateWithFlags(&h_, timing ? hipEventDefault : hipEventDisableTiming)); }
};

}  // namespace zkp
