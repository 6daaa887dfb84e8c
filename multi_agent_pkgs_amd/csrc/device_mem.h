// device_mem.h — who owns device memory and HIP events in the host code outside the solver handle: DevBuf<T> one hipMalloc block,
// DevEvent one hipEvent_t, TimedInterval two events round a stretch of a stream; FirstError is the "first error wins" of the batch
// entry points. The owners are move-only members or locals: what is not moved out is released where it goes out of scope.
#pragma once
#include <cstddef>
#include <utility>

#ifdef HDSM_DEVICE_MEM_HOST
// Test seam (tests/device_mem_check.cpp): allocation, fill, release and the events' lifetime on host memory, with a count of what is
// live and a knob that fails the k-th allocation from now. Only the types of the HIP runtime are used, nothing of it is linked.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
namespace hdsm_mem {
inline long g_live = 0;     // blocks and events allocated and not yet released
inline long g_fail_in = 0;  // k > 0: the k-th allocation from now fails (once)
inline hipError_t raw_alloc(void** p, size_t bytes) {
  const bool refuse = g_fail_in > 0 && --g_fail_in == 0;
  *p = refuse ? nullptr : std::malloc(bytes);
  g_live += *p != nullptr;
  return *p != nullptr ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t raw_fill(void* p, int v, size_t bytes) { return std::memset(p, v, bytes), hipSuccess; }
inline hipError_t raw_free(void* p) { return std::free(p), --g_live, hipSuccess; }
inline hipError_t raw_event_create(hipEvent_t* e) { return raw_alloc(reinterpret_cast<void**>(e), 1); }
inline hipError_t raw_event_destroy(hipEvent_t e) { return raw_free(e); }
}  // namespace hdsm_mem
#else
#include <hip/hip_runtime.h>
namespace hdsm_mem {
inline hipError_t raw_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t raw_fill(void* p, int v, size_t bytes) { return hipMemset(p, v, bytes); }
inline hipError_t raw_free(void* p) { return hipFree(p); }
inline hipError_t raw_event_create(hipEvent_t* e) { return hipEventCreate(e); }
inline hipError_t raw_event_destroy(hipEvent_t e) { return hipEventDestroy(e); }
}  // namespace hdsm_mem
#endif

namespace hdsm_mem __attribute__((visibility("hidden"))) {  // (inline helpers of the host code: libhdsm.so exports none of them)

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) reset(), p_ = std::exchange(o.p_, nullptr);
    return *this;
  }
  ~DevBuf() { reset(); }
  // `count` elements (at least one) in place of what was held; after an error the buffer is empty
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = raw_alloc(reinterpret_cast<void**>(&p_), (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  hipError_t alloc_zeroed(size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : raw_fill(p_, 0, (count ? count : 1) * sizeof(T));
  }
  T* get() const { return p_; }
  void reset() {
    if (p_) (void)raw_free(std::exchange(p_, nullptr));
  }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
};

class DevEvent {  // created by the first create(), not by the constructor: an object that never times anything holds no event
 public:
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) reset(), e_ = std::exchange(o.e_, nullptr);
    return *this;
  }
  ~DevEvent() { reset(); }
  hipError_t create() { return e_ ? hipSuccess : raw_event_create(&e_); }
  hipEvent_t get() const { return e_; }
  void reset() {
    if (e_) (void)raw_event_destroy(std::exchange(e_, nullptr));
  }
  explicit operator bool() const { return e_ != nullptr; }

 private:
  hipEvent_t e_ = nullptr;
};

// A stretch of a stream between two records. `valid`: the last round recorded both (whoever starts a round clears it).
struct TimedInterval {
  DevEvent start, stop;
  bool valid = false;
  hipError_t create() {
    const hipError_t e = start.create();
    return e != hipSuccess ? e : stop.create();
  }
  hipError_t record_start(hipStream_t st) { return hipEventRecord(start.get(), st); }
  hipError_t record_stop(hipStream_t st) {
    const hipError_t e = hipEventRecord(stop.get(), st);
    valid = e == hipSuccess;
    return e;
  }
  // milliseconds between the two records, after waiting for the second; refuses (and leaves *out alone) when not valid
  hipError_t ms(float* out) const {
    if (!valid) return hipErrorNotReady;
    const hipError_t e = hipEventSynchronize(stop.get());
    return e != hipSuccess ? e : hipEventElapsedTime(out, start.get(), stop.get());
  }
};

struct FirstError {  // err(call), err(call), ...: keeps the first error
  hipError_t e = hipSuccess;
  void operator()(hipError_t r) {
    if (e == hipSuccess) e = r;
  }
  bool ok() const { return e == hipSuccess; }
};

}  // namespace hdsm_mem
