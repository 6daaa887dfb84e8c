// hdsm_entry.h — private host header of the hdsm_ entry points: what hdsm_api.hip, reference_kernels.hip, exchange_kernels.hip and
// replan_host.hip share and nothing else. They report through ONE error text (hdsm_last_error); the helpers below touch only
// members of the handle. Not for hdsm_handle.h: that header stays free of runtime calls (g++ compiles it for the tests).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/hdsm.h"
#include "hdsm_handle.h"

namespace hdsm_entry __attribute__((visibility("hidden"))) {

using hdsm_handle::Handle;

// (hdsm_api.hip, next to the thread's error text)
int set_err(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      (void)hipGetLastError(); /* reported here: the next call must not trip over it again */            \
      return set_err(HDSM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    }                                                                                                   \
  } while (0)

// (hdsm_api.hip, next to launch_rescue) hdsm_replan knows at once whether an instance ran out of staging rows: if the last launch
// on `st` used a shared-CU kernel and carried no rescue pass, wait for it and, if the word is up, solve those instances again now
int rescue_if_flagged(Handle* h, hipStream_t st);

// The handle's device state (snapshots, warm-start sets, prefilter records, staging buffers) is shared by all its calls: one that
// arrives on another stream than the previous launch waits for it. (Who launches on `st` also names it as last_stream; who only
// stages into the handle's buffers does not.) The event it waits for is recorded HERE, at the tail of last_stream — at or after the
// handle's last launch, which is all the wait needs — and not after every launch: a caller that stays on one stream (the documented
// normal case) never puts a record, a barrier packet in front of its next kernel, on its queue. last_stream must still be alive.
inline hipError_t join_stream(Handle* h, hipStream_t st) {
  if (!h->launched || st == h->last_stream) return hipSuccess;
  if (h->done_pending) {
    if (const hipError_t e = hipEventRecord(h->ev_done.get(), h->last_stream)) return e;
    h->done_pending = false;
  }
  return hipStreamWaitEvent(st, h->ev_done.get(), 0);
}

// ... and this is the point it waits for: the end of what a device entry point enqueued on last_stream (nothing is recorded here)
inline hipError_t mark_done(Handle* h, hipStream_t st) {
  (void)st;
  h->launched = true, h->done_pending = true;
  return hipSuccess;
}

// stream-ordered copies of a host-pointer entry point: nothing to do for zero bytes, and nothing more after the first error
struct Copies {
  hipStream_t st;
  hdsm_mem::FirstError err;
  void operator()(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (err.ok() && bytes) err(hipMemcpyAsync(dst, src, bytes, kind, st));
  }
};

inline int check_common(Handle* h, int n_inst, int n_rob) {
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  if (n_inst < 0 || n_rob < 0) return set_err(HDSM_ERR_BAD_ARG, "negative size");
  if (n_inst > h->max_inst) return set_err(HDSM_ERR_CAPACITY, "n_inst exceeds max_instances of the handle");
  if (n_rob > h->n_rob_max) return set_err(HDSM_ERR_CAPACITY, "n_rob exceeds n_rob_max of the handle");
  return HDSM_OK;
}

// ... and for the entry points that enumerate neighbours: a partition (hdsm_set_groups) must lie inside the call's n_rob
inline int check_neighbours(Handle* h, int n_inst, int n_rob) {
  if (int rc = check_common(h, n_inst, n_rob)) return rc;
  if (n_rob < h->n_total) return set_err(HDSM_ERR_BAD_ARG, "n_rob is smaller than the agents of the partition (hdsm_set_groups)");
  return HDSM_OK;
}

}  // namespace hdsm_entry
