// device_mem.h — who owns device memory, pinned host memory, streams and HIP events in the host code: DevBuf<T> one hipMalloc block,
// GrowBuf<T> one that grows on demand, PinnedBuf a grow-only page-locked host block, MappedWord one int32 both sides see, DevStream one
// stream, DevEvent one hipEvent_t, TimedInterval two events round a stretch of a stream; FirstError is the "first error wins" of the
// batch entry points. The owners are move-only members or locals: what is not moved out is released where it goes out of scope.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>

#ifdef HDSM_DEVICE_MEM_HOST
// Test seam (tests/device_mem_check.cpp): allocation, fill, release and the lifetime of events and streams on host memory, with a
// count of what is live and a knob that fails the k-th allocation from now. Only the types of the HIP runtime are used, nothing of
// it is linked.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
namespace hdsm_mem {
inline long g_live = 0;     // blocks, events and streams allocated and not yet released
inline long g_fail_in = 0;  // k > 0: the k-th allocation from now fails (once)
inline long g_syncs = 0;    // stream synchronisations so far
inline hipError_t raw_alloc(void** p, size_t bytes) {
  const bool refuse = g_fail_in > 0 && --g_fail_in == 0;
  *p = refuse ? nullptr : std::malloc(bytes);
  g_live += *p != nullptr;
  return *p != nullptr ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t raw_fill(void* p, int v, size_t bytes) { return std::memset(p, v, bytes), hipSuccess; }
inline hipError_t raw_free(void* p) { return std::free(p), --g_live, hipSuccess; }
inline hipError_t raw_host_alloc(void** p, size_t bytes, unsigned) { return raw_alloc(p, bytes); }
inline hipError_t raw_host_free(void* p) { return raw_free(p); }
inline hipError_t raw_host_alias(void** dev, void* host) { return *dev = host, hipSuccess; }
inline hipError_t raw_event_create(hipEvent_t* e, unsigned) { return raw_alloc(reinterpret_cast<void**>(e), 1); }
inline hipError_t raw_event_destroy(hipEvent_t e) { return raw_free(e); }
inline hipError_t raw_stream_create(hipStream_t* s) { return raw_alloc(reinterpret_cast<void**>(s), 1); }
inline hipError_t raw_stream_destroy(hipStream_t s) { return raw_free(s); }
inline hipError_t raw_stream_sync(hipStream_t) { return ++g_syncs, hipSuccess; }
}  // namespace hdsm_mem
#else
#include <hip/hip_runtime.h>
namespace hdsm_mem {
inline hipError_t raw_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t raw_fill(void* p, int v, size_t bytes) { return hipMemset(p, v, bytes); }
inline hipError_t raw_free(void* p) { return hipFree(p); }
inline hipError_t raw_host_alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
inline hipError_t raw_host_free(void* p) { return hipHostFree(p); }
inline hipError_t raw_host_alias(void** dev, void* host) { return hipHostGetDevicePointer(dev, host, 0); }
inline hipError_t raw_event_create(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
inline hipError_t raw_event_destroy(hipEvent_t e) { return hipEventDestroy(e); }
inline hipError_t raw_stream_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
inline hipError_t raw_stream_destroy(hipStream_t s) { return hipStreamDestroy(s); }
inline hipError_t raw_stream_sync(hipStream_t s) { return hipStreamSynchronize(s); }
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

// Grow-only device scratch: reallocated, after draining the stream that may still be using it, only when a call needs more than any
// before. After a failed allocation it is empty with capacity 0.
template <class T>
class GrowBuf {
 public:
  GrowBuf() = default;
  GrowBuf(GrowBuf&& o) noexcept : b_(std::move(o.b_)), cap_(std::exchange(o.cap_, 0)) {}
  GrowBuf& operator=(GrowBuf&& o) noexcept {
    if (this != &o) b_ = std::move(o.b_), cap_ = std::exchange(o.cap_, 0);
    return *this;
  }
  hipError_t ensure(size_t count, hipStream_t drain) {
    if (count <= cap_) return hipSuccess;
    hipError_t e = raw_stream_sync(drain);
    if (e != hipSuccess) return e;
    cap_ = 0;
    e = b_.alloc(count);
    if (e == hipSuccess) cap_ = count;
    return e;
  }
  T* get() const { return b_.get(); }
  size_t capacity() const { return cap_; }

 private:
  DevBuf<T> b_;
  size_t cap_ = 0;
};

class PinnedBuf {  // a grow-only block of page-locked host memory; after a failed allocation it is empty with capacity 0
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) reset(), p_ = std::exchange(o.p_, nullptr), cap_ = std::exchange(o.cap_, 0);
    return *this;
  }
  ~PinnedBuf() { reset(); }
  hipError_t ensure(size_t bytes, unsigned flags = hipHostMallocDefault) {
    if (bytes <= cap_) return hipSuccess;
    reset();
    const hipError_t e = raw_host_alloc(&p_, bytes, flags);
    if (e != hipSuccess) p_ = nullptr;
    else cap_ = bytes;
    return e;
  }
  void* get() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) (void)raw_host_free(std::exchange(p_, nullptr));
    cap_ = 0;
  }

 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};

class MappedWord {  // one int32 in mapped page-locked host memory, zero at first: kernels write it through dev(), the host reads host()
 public:
  hipError_t create() {
    hipError_t e = w_.ensure(sizeof(int32_t), hipHostMallocMapped);
    if (e != hipSuccess) return e;
    *host() = 0;
    e = raw_host_alias(reinterpret_cast<void**>(&d_), w_.get());
    if (e != hipSuccess) w_.reset(), d_ = nullptr;
    return e;
  }
  int32_t* host() const { return static_cast<int32_t*>(w_.get()); }
  int32_t* dev() const { return host() ? d_ : nullptr; }

 private:
  PinnedBuf w_;
  int32_t* d_ = nullptr;  // (means something only while w_ holds the word)
};

class DevStream {  // one non-blocking stream
 public:
  DevStream() = default;
  DevStream(DevStream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  DevStream& operator=(DevStream&& o) noexcept {
    if (this != &o) reset(), s_ = std::exchange(o.s_, nullptr);
    return *this;
  }
  ~DevStream() { reset(); }
  hipError_t create() { return s_ ? hipSuccess : raw_stream_create(&s_); }
  hipStream_t get() const { return s_; }
  void reset() {
    if (s_) (void)raw_stream_destroy(std::exchange(s_, nullptr));
  }

 private:
  hipStream_t s_ = nullptr;
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
  hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : raw_event_create(&e_, flags); }
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
