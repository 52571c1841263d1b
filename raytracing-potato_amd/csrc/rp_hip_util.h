// rp_hip_util.h -- what the C-ABI's translation units (rp_scene.cpp, rp_render.cpp, rp_gather.cpp) share, and of which
// the device tree builder (rp_bvh_gpu.hip) uses the owner of device memory: the error
// slot, the HIP / RCCL call checks, and the owners of device memory, streams, events and communicators.  Internal to
// librp.so: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <memory>
#include <string>
#include <utility>

#include "../../include/rp.h"

#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;  // rp_last_error's message, one per thread (defined in rp_scene.cpp)

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define RP_HIP(call)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail(RP_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define RP_NCCL(call)                                                                           \
  do {                                                                                          \
    ncclResult_t r_ = (call);                                                                   \
    if (r_ != ncclSuccess) return fail(RP_ERCCL, std::string(#call) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// A rpk::launch_* call (rp_kernel.h: a hipError_t as int).
#define RP_LAUNCH(what, call)                                                                                  \
  do {                                                                                                         \
    int l_ = (call);                                                                                           \
    if (l_ != 0) return fail(RP_EHIP, std::string(what " launch: ") + hipGetErrorString((hipError_t)l_));      \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Device memory of `capacity()` elements of T, freed with its owner (on the device current then: see Guarded).
template <class T>
class DevBuf {
  T* p_ = nullptr;
  uint64_t cap_ = 0;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // n elements (at least one is allocated), uninitialised; false: hipMalloc failed (*err: with what) and the buffer
  // is empty
  bool alloc(uint64_t n, hipError_t* err = nullptr) {
    reset();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * (n ? n : 1));
    if (err) *err = e;
    if (e != hipSuccess) {
      p_ = nullptr;
      return false;
    }
    cap_ = n;
    return true;
  }
  // grow only: the old buffer is freed, then the new one allocated (synchronous, nothing copied)
  bool reserve(uint64_t n) { return n <= cap_ || alloc(n); }
  // take over a hipMalloc'ed pointer (the device tree builder's outputs)
  void adopt(T* p, uint64_t n) {
    reset();
    p_ = p;
    cap_ = n;
  }
  // hand the pointer out: the caller frees it (the device tree builder's outputs leave it this way)
  T* release() {
    cap_ = 0;
    return std::exchange(p_, nullptr);
  }
  T* get() const { return p_; }
  uint64_t capacity() const { return cap_; }
};

// A stream, event or communicator destroyed with its owner.
template <class H, auto Destroy>
class Handle {
  H h_ = nullptr;

 public:
  Handle() = default;
  explicit Handle(H h) : h_(h) {}
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  ~Handle() {
    if (h_) (void)Destroy(h_);
  }
  H get() const { return h_; }
  H* put() { return &h_; }  // for the create call of an empty handle
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Comm = Handle<ncclComm_t, ncclCommDestroy>;

// An object whose device resources are released on its own device: T has an `int device`.
struct GuardedDelete {
  template <class T>
  void operator()(T* p) const {
    DeviceGuard g(p->device);
    delete p;
  }
};
template <class T>
using Guarded = std::unique_ptr<T, GuardedDelete>;

#pragma GCC visibility pop
