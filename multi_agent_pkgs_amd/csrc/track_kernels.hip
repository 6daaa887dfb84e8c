// track_kernels.hip — imperfect tracking (track_core.h) on the device, for hdsm_track_states_batch and the device-resident loop:
//   k_track   one lane per agent, 64-lane workgroups. Model form: the lane reads traj_curr[step_plan] of its AgentS, writes the flown
//             state into state_curr and books the difference in the agent's hdsm_track_record. External form: the lane reads its row
//             of the supplied states instead and books against the state it replaces. Batch form: ids, planned and flown arrays.
// In the loop it runs right behind k_commit on the same stream. No LDS, no scratch, no atomics — an agent's state and record have one
// owner; the arithmetic is track_core.h's, the same source as the host forms.
#include <hip/hip_runtime.h>

#include "../../include/hdsm_swarm.h"
#include "device_mem.h"
#include "hdsm_internal.h"
#include "track_core.h"
#include "track_device.h"

namespace hdsm_track {
namespace {

__global__ __launch_bounds__(64) void k_track(Launch a) {
  const int k = (int)(blockIdx.x * 64u + threadIdx.x);
  if (k >= a.n) return;
  double from[9], to[9];
  if (a.agents == nullptr) {  // batch
    const double* in = a.planned + (size_t)k * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) from[c] = in[c];
    flown_state(a.model, a.ids[k], a.q, a.T, from, to);
    double* out = a.flown + (size_t)k * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) out[c] = to[c];
    if (a.dist != nullptr) a.dist[k] = pos_dist(from, to);
    return;
  }
  hdsm_sw::AgentS& ag = a.agents[k];
  const bool external = a.src != nullptr;
  if (external) {
    if (a.mask != nullptr && a.mask[k] == 0) return;
    const double* in = a.src + (size_t)k * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) to[c] = in[c];
    if (!finite9(to)) return;
#pragma unroll
    for (int c = 0; c < 9; ++c) from[c] = ag.state_curr[c];
  } else {
    if (ag.has_traj == 0) return;
    const double* in = ag.traj_curr[a.step_plan];
#pragma unroll
    for (int c = 0; c < 9; ++c) from[c] = in[c];
    flown_state(a.model, ag.id, a.q, a.T, from, to);
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) ag.state_curr[c] = to[c];
  if (a.hist_row != nullptr) {
    double* row = a.hist_row + (size_t)k * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = to[c];
  }
  hdsm_track_record r = a.records[k];
  book(r, pos_dist(from, to), vel_dist(from, to), external);
  a.records[k] = r;
}

}  // namespace

hipError_t launch(const Launch& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_track, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace hdsm_track

extern "C" int hdsm_track_states_batch(int32_t device, const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T,
                                       int64_t round, double* flown, double* dist) {
  const int rc = hdsm_internal_track_args(m, n, agent_id, planned, T, round, flown);
  if (rc) return rc;
  if (n == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t count = (size_t)n * 9;
  hdsm_mem::DevBuf<int32_t> d_ids;
  hdsm_mem::DevBuf<double> d_planned, d_flown, d_dist;
  hdsm_mem::FirstError ok;
  ok(d_ids.alloc((size_t)n)), ok(d_planned.alloc(count)), ok(d_flown.alloc(count)), ok(d_dist.alloc((size_t)n));
  if (ok.ok()) ok(hipMemcpy(d_ids.get(), agent_id, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  if (ok.ok()) ok(hipMemcpy(d_planned.get(), planned, count * sizeof(double), hipMemcpyHostToDevice));
  if (ok.ok()) {
    ok(hdsm_track::launch(hdsm_track::Launch{n, 0, (long long)round, T, *m, nullptr, nullptr, nullptr, nullptr, d_ids.get(), d_planned.get(),
                                             d_flown.get(), d_dist.get(), nullptr},
                          nullptr));
    ok(hipDeviceSynchronize());
  }
  if (ok.ok()) ok(hipMemcpy(flown, d_flown.get(), count * sizeof(double), hipMemcpyDeviceToHost));
  if (ok.ok() && dist) ok(hipMemcpy(dist, d_dist.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}
