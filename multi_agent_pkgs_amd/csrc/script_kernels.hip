// script_kernels.hip — scripted agents (script_core.h) on the device, for hdsm_script_records_batch and the device-resident loop:
//   k_script   one wavefront per scripted slot, one state of the record per lane (N + 1 <= 17 of the 64): the lane forms its state
//              from the track and writes its nine doubles of the published record. In the loop the same lanes write the agent's
//              traj_curr, the lane of state step_plan its state_curr, lane 0 the flag, the status, has_traj and the goal (the last
//              knot) — so the history, the audit, the group report and a download see a scripted agent like any other.
// It runs right behind k_commit on the same stream and overwrites the slots k_commit has just padded. No LDS, no scratch, no atomics;
// the arithmetic is script_core.h's, the same source as the host form.
#include <hip/hip_runtime.h>

#include "../../include/hdsm_swarm.h"
#include "device_mem.h"
#include "hdsm_internal.h"
#include "script_core.h"
#include "script_device.h"

namespace hdsm_script {
namespace {

__global__ __launch_bounds__(64) void k_script(Round r) {
  const int k = (int)blockIdx.x, i = (int)threadIdx.x;
  if (k >= r.n_script) return;
  const double* knots = r.knots + (size_t)k * r.n_knots * 4;
  if (i <= r.N) {
    double s[9];
    record_state(knots, r.n_knots, r.step_plan, r.dt, r.predict, r.round, i, s);
    double* out = r.records + ((size_t)k * (r.N + 1) + i) * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) out[c] = s[c];
    if (r.agents != nullptr) {
      hdsm_sw::AgentS& ag = r.agents[k];
#pragma unroll
      for (int c = 0; c < 9; ++c) ag.traj_curr[i][c] = s[c];
      if (i == r.step_plan) {
#pragma unroll
        for (int c = 0; c < 9; ++c) ag.state_curr[c] = s[c];
      }
    }
  }
  if (i == 0) {
    if (r.agents != nullptr) {
      hdsm_sw::AgentS& ag = r.agents[k];
      const double* last = knots + 4 * (size_t)(r.n_knots - 1);
      ag.has_traj = 1;
      ag.goal = hdsm_sw::V3{{last[1], last[2], last[3]}};
    }
    if (r.has != nullptr) r.has[k] = 1;
    if (r.status != nullptr) r.status[k] = HDSM_OK;
  }
}

}  // namespace

hipError_t launch(const Round& r, hipStream_t st) {
  if (r.n_script <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_script, dim3((unsigned)r.n_script), dim3(64), 0, st, r);
  return hipGetLastError();
}

}  // namespace hdsm_script

extern "C" int hdsm_script_records_batch(int32_t device, int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan,
                                         double dt, int32_t predict, int64_t round, double* records) {
  const int rc = hdsm_internal_script_args(n_script, n_knots, knots, n_hor, step_plan, dt, predict, round, records);
  if (rc) return rc;
  if (n_script == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t kcount = (size_t)n_script * n_knots * 4, rcount = (size_t)n_script * (n_hor + 1) * 9;
  hdsm_mem::DevBuf<double> d_knots, d_records;
  hdsm_mem::FirstError ok;
  ok(d_knots.alloc(kcount)), ok(d_records.alloc(rcount));
  if (ok.ok()) ok(hipMemcpy(d_knots.get(), knots, kcount * sizeof(double), hipMemcpyHostToDevice));
  if (ok.ok()) {
    ok(hdsm_script::launch(hdsm_script::Round{n_script, n_knots, n_hor, step_plan, predict, (long long)round, dt, d_knots.get(), d_records.get(), nullptr,
                                              nullptr, nullptr},
                           nullptr));
    ok(hipDeviceSynchronize());
  }
  if (ok.ok()) ok(hipMemcpy(records, d_records.get(), rcount * sizeof(double), hipMemcpyDeviceToHost));
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}
