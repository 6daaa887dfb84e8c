// command_kernels.hip — commands for the vehicle (command_core.h) on the device, for hdsm_command_batch and the device-resident loop:
//   k_command   one lane per agent, 64-lane workgroups. Loop form: the lane reads state_curr of before the commit from the solver's x_0
//               input, the reference point from this round's reference buffer, the record and the state the round ends in from its
//               committed AgentS, steps the agent's yaw and writes step_plan setpoints and the pose. Batch form: plain arrays.
// In the loop it is the last launch of phase [5], behind k_commit, k_track and k_script on the same stream. No LDS, no scratch; an
// agent's yaw and records have one owner; the two counters take one atomic add per wavefront. The arithmetic is command_core.h's,
// the same source as the host forms.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/hdsm_swarm.h"
#include "command_core.h"
#include "command_device.h"
#include "device_mem.h"
#include "hdsm_internal.h"

namespace hdsm_cmd {
namespace {

__global__ __launch_bounds__(64) void k_command(Launch a) {
  const int k = (int)(blockIdx.x * 64u + threadIdx.x);
  const bool live = k < a.n;
  int stepped = 0, flown = 0;
  if (live) {
    hdsm_command* const sp = a.setpoint != nullptr ? a.setpoint + (size_t)k * a.step_plan : nullptr;
    hdsm_command* const po = a.pose != nullptr ? a.pose + k : nullptr;
    if (a.agents == nullptr) {  // batch
      flown = 1;
      a.yaw[k] = agent_round(a.yaw[k], a.n_ref[k] > a.yaw_idx, a.ref_point + (size_t)k * 3, a.before + (size_t)k * 9,
                             a.records + (size_t)k * (a.N + 1) * 9, a.after + (size_t)k * 9, a.valid_in[k], a.step_plan, a.k_p_yaw, a.dt, sp, po,
                             &stepped);
    } else if (k < a.n_fly) {
      flown = 1;
      const hdsm_sw::AgentS& ag = a.agents[k];
      // Everything the lane reads is asked for up front and without a condition (all of it is in bounds whatever the agent's state): behind
      // the branches of the yaw step the loads would follow one another, a memory round trip each, and those are the kernel's time.
      const double* const rp = a.ref_full + ((size_t)k * (a.N + 1) + a.yaw_idx) * 6;
      const double* const bp = a.before + (size_t)k * 9;
      const double ref[3] = {rp[0], rp[1], rp[2]}, before[3] = {bp[0], bp[1], bp[2]};
      const double yaw = a.yaw[k];
      const int has_traj = ag.has_traj, st = a.status[k];
      double after[9], rec[18];  // (rec: knots 0 and 1 of the record; knot 0 is never read)
#pragma unroll
      for (int c = 0; c < 9; ++c) after[c] = ag.state_curr[c], rec[c] = 0.0, rec[9 + c] = ag.traj_curr[1][c];
      const int valid = has_traj == 0 ? 0 : (st != HDSM_NO_SOLUTION ? 1 : 2);
      const bool has_ref = a.N + 1 > a.yaw_idx;
      if (a.step_plan == 1) a.yaw[k] = agent_round(yaw, has_ref, ref, before, rec, after, valid, 1, a.k_p_yaw, a.dt, sp, po, &stepped);
      else a.yaw[k] = agent_round(yaw, has_ref, ref, before, &ag.traj_curr[0][0], after, valid, a.step_plan, a.k_p_yaw, a.dt, sp, po, &stepped);
    } else {  // the scripted tail
      hdsm_command c;
      zero(c);
      for (int j = 0; j < a.step_plan; ++j) sp[j] = c;
      *po = c;
    }
  }
  if (a.cnt != nullptr) {
    const int took = __popcll(__ballot(flown != 0 && stepped != 0)), skipped = __popcll(__ballot(flown != 0 && stepped == 0));
    if (threadIdx.x == 0) {
      if (took) atomicAdd(&a.cnt[0], (unsigned long long)took);
      if (skipped) atomicAdd(&a.cnt[1], (unsigned long long)skipped);
    }
  }
}

}  // namespace

hipError_t launch(const Launch& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_command, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace hdsm_cmd

extern "C" int hdsm_command_batch(int32_t device, int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw,
                                  const int32_t* n_ref, const double* ref_point, const double* state_before, const double* records,
                                  const int32_t* valid_in, const double* state_after, double* yaw, hdsm_command* setpoint, hdsm_command* pose,
                                  int64_t stats[2]) {
  const int rc = hdsm_internal_command_args(n, n_hor, step_plan, dt, yaw_idx, k_p_yaw, n_ref, ref_point, state_before, records, valid_in,
                                            state_after, yaw);
  if (rc) return rc;
  if (n == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t N = (size_t)n, rec = (size_t)(n_hor + 1) * 9;
  hdsm_mem::DevBuf<int32_t> d_nref, d_valid;
  hdsm_mem::DevBuf<double> d_ref, d_before, d_rec, d_after, d_yaw;
  hdsm_mem::DevBuf<hdsm_command> d_sp, d_pose;
  hdsm_mem::DevBuf<unsigned long long> d_cnt;
  hdsm_mem::FirstError ok;
  ok(d_nref.alloc(N)), ok(d_valid.alloc(N)), ok(d_ref.alloc(N * 3)), ok(d_before.alloc(N * 9)), ok(d_rec.alloc(N * rec)), ok(d_after.alloc(N * 9));
  ok(d_yaw.alloc(N)), ok(d_sp.alloc(N * (size_t)step_plan)), ok(d_pose.alloc(N)), ok(d_cnt.alloc_zeroed(2));
  const auto up = [&](void* dst, const void* src, size_t bytes) {
    if (ok.ok()) ok(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  };
  up(d_nref.get(), n_ref, N * 4), up(d_valid.get(), valid_in, N * 4), up(d_ref.get(), ref_point, N * 3 * 8), up(d_before.get(), state_before, N * 9 * 8);
  up(d_rec.get(), records, N * rec * 8), up(d_after.get(), state_after, N * 9 * 8), up(d_yaw.get(), yaw, N * 8);
  if (ok.ok()) {
    ok(hipDeviceSynchronize());  // (the counters' fill is done)
    hdsm_cmd::Launch a{};
    a.n = n, a.n_fly = n, a.N = n_hor, a.step_plan = step_plan, a.yaw_idx = yaw_idx, a.dt = dt, a.k_p_yaw = k_p_yaw;
    a.n_ref = d_nref.get(), a.ref_point = d_ref.get(), a.before = d_before.get(), a.records = d_rec.get(), a.valid_in = d_valid.get();
    a.after = d_after.get(), a.yaw = d_yaw.get(), a.setpoint = d_sp.get(), a.pose = d_pose.get(), a.cnt = d_cnt.get();
    ok(hdsm_cmd::launch(a, nullptr));
    ok(hipDeviceSynchronize());
  }
  const auto down = [&](void* dst, const void* src, size_t bytes) {
    if (ok.ok() && dst) ok(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  };
  down(yaw, d_yaw.get(), N * 8), down(setpoint, d_sp.get(), N * (size_t)step_plan * sizeof(hdsm_command)), down(pose, d_pose.get(), N * sizeof(hdsm_command));
  unsigned long long cnt[2] = {0, 0};
  down(cnt, d_cnt.get(), sizeof cnt);
  if (ok.ok() && stats) stats[0] += (int64_t)cnt[0], stats[1] += (int64_t)cnt[1];
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}
