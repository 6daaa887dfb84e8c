// vehicle_kernels.hip — a vehicle in the loop (vehicle_core.h) on the device, for hdsm_vehicle_fly_batch and the device-resident loop:
//   k_vehicle   one lane per flown agent, 64-lane workgroups. Loop form: the lane reads its vehicle state, the setpoints k_command has
//               just written, knot 0 (traj_curr[0]) and the committed state_curr of its AgentS, flies step_plan * n_sub sub-steps — a
//               controller evaluation and one RK4 step each, a dependent chain — and writes the vehicle state, state_curr, the agent's
//               track record and its pose. Batch form: plain arrays.
//   k_seat      one lane per agent: a vehicle seated on a given state and the agent's yaw (the first switch-on, states from outside).
// In the loop k_vehicle is the last launch of phase [5], behind k_command on the same stream. No LDS, no scratch; an agent's vehicle,
// state, record and pose have one owner; the four counters take one atomic add per wavefront. The arithmetic is vehicle_core.h's, the
// same source as the host forms.
#include <hip/hip_runtime.h>

#include "../../include/hdsm_swarm.h"
#include "device_mem.h"
#include "hdsm_internal.h"
#include "vehicle_core.h"
#include "vehicle_device.h"

namespace hdsm_veh {
namespace {

// the sum of v over the wavefront's 64 lanes, in every lane (cross-lane moves: no LDS is allocated)
__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(64) void k_vehicle(Launch a) {
  const int k = (int)(blockIdx.x * 64u + threadIdx.x);
  int flew = 0, reseated = 0, n_thrust = 0, n_rate = 0;
  if (k < a.n) {
    // Everything the lane reads is asked for up front and without a condition: the sub-steps are one dependent chain, and a load behind
    // a branch would be a memory round trip added to it. (The setpoints behind the first are asked for one interval ahead.)
    const hdsm_vehicle_state vin = a.vstate[k];
    hdsm_vehicle_state vs = vin;
    const hdsm_command* const sp = a.setpoint + (size_t)k * a.step_plan;
    hdsm_sw::AgentS* const ag = a.agents != nullptr ? a.agents + k : nullptr;
    const double* const sp0 = ag != nullptr ? &ag->traj_curr[0][0] : a.start + (size_t)k * 9;
    const double* const pe = ag != nullptr ? &ag->state_curr[0] : a.planned_end + (size_t)k * 9;
    const int32_t id = ag != nullptr ? ag->id : a.ids[k];
    double start[9], planned[9], flown[9], d, dvel;
#pragma unroll
    for (int c = 0; c < 9; ++c) start[c] = sp0[c], planned[c] = pe[c];
    hdsm_track_record rec{};
    if (ag != nullptr) rec = a.records[k];
    const int ok = agent_round(a.m, id, a.q, a.step_plan, a.dt, start, sp, planned, vs, flown, &d, &dvel, a.pose != nullptr ? a.pose + k : nullptr,
                               &n_thrust, &n_rate);
    flew = ok, reseated = 1 - ok;
    a.vstate[k] = vs;
    if (ag != nullptr) {
#pragma unroll
      for (int c = 0; c < 9; ++c) ag->state_curr[c] = flown[c];
      if (ok) {
        hdsm_track::book(rec, d, dvel, false);
        a.records[k] = rec;
      }
    } else {
      double* out = a.flown + (size_t)k * 9;
#pragma unroll
      for (int c = 0; c < 9; ++c) out[c] = flown[c];
      if (a.dist != nullptr) a.dist[k] = d;
    }
  }
  if (a.cnt != nullptr) {
    const int s0 = wave_sum(flew), s1 = wave_sum(reseated), s2 = wave_sum(n_thrust), s3 = wave_sum(n_rate);
    if (threadIdx.x == 0) {
      if (s0) atomicAdd(&a.cnt[0], (unsigned long long)s0);
      if (s1) atomicAdd(&a.cnt[1], (unsigned long long)s1);
      if (s2) atomicAdd(&a.cnt[2], (unsigned long long)s2);
      if (s3) atomicAdd(&a.cnt[3], (unsigned long long)s3);
    }
  }
}

__global__ __launch_bounds__(64) void k_seat(Seat a) {
  const int k = (int)(blockIdx.x * 64u + threadIdx.x);
  if (k >= a.n) return;
  if (a.mask != nullptr && a.mask[k] == 0) return;
  const double* in = a.states + (size_t)k * a.stride;
  double s[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) s[c] = in[c];
  if (!hdsm_track::finite9(s)) return;
  hdsm_vehicle_state vs;
  seat(a.m, s, a.yaw[k], vs);
  a.vstate[k] = vs;
}

}  // namespace

hipError_t launch(const Launch& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vehicle, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_seat(const Seat& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_seat, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace hdsm_veh

extern "C" int hdsm_vehicle_fly_batch(int32_t device, const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt,
                                      int64_t round, const double* start, const hdsm_command* setpoint, const double* planned_end,
                                      hdsm_vehicle_state* vstate, double* flown, double* dist, hdsm_command* pose, int64_t stats[4]) {
  const int rc = hdsm_internal_vehicle_args(m, n, agent_id, step_plan, dt, round, start, setpoint, planned_end, vstate, flown);
  if (rc) return rc;
  if (n == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t N = (size_t)n;
  hdsm_mem::DevBuf<int32_t> d_ids;
  hdsm_mem::DevBuf<double> d_start, d_end, d_flown, d_dist;
  hdsm_mem::DevBuf<hdsm_command> d_sp, d_pose;
  hdsm_mem::DevBuf<hdsm_vehicle_state> d_vs;
  hdsm_mem::DevBuf<unsigned long long> d_cnt;
  hdsm_mem::FirstError ok;
  ok(d_ids.alloc(N)), ok(d_start.alloc(N * 9)), ok(d_end.alloc(N * 9)), ok(d_flown.alloc(N * 9)), ok(d_dist.alloc(N));
  ok(d_sp.alloc(N * (size_t)step_plan)), ok(d_pose.alloc(N)), ok(d_vs.alloc(N)), ok(d_cnt.alloc_zeroed(4));
  const auto up = [&](void* dst, const void* src, size_t bytes) {
    if (ok.ok()) ok(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  };
  up(d_ids.get(), agent_id, N * 4), up(d_start.get(), start, N * 9 * 8), up(d_end.get(), planned_end, N * 9 * 8);
  up(d_sp.get(), setpoint, N * (size_t)step_plan * sizeof(hdsm_command)), up(d_vs.get(), vstate, N * sizeof(hdsm_vehicle_state));
  if (ok.ok()) {
    ok(hipDeviceSynchronize());  // (the counters' fill is done)
    hdsm_veh::Launch a{};
    a.n = n, a.step_plan = step_plan, a.q = (long long)round, a.dt = dt, a.m = *m;
    a.ids = d_ids.get(), a.start = d_start.get(), a.planned_end = d_end.get(), a.flown = d_flown.get(), a.dist = d_dist.get();
    a.setpoint = d_sp.get(), a.vstate = d_vs.get(), a.pose = d_pose.get(), a.cnt = d_cnt.get();
    ok(hdsm_veh::launch(a, nullptr));
    ok(hipDeviceSynchronize());
  }
  const auto down = [&](void* dst, const void* src, size_t bytes) {
    if (ok.ok() && dst) ok(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  };
  down(vstate, d_vs.get(), N * sizeof(hdsm_vehicle_state)), down(flown, d_flown.get(), N * 9 * 8), down(dist, d_dist.get(), N * 8);
  down(pose, d_pose.get(), N * sizeof(hdsm_command));
  unsigned long long cnt[4] = {0, 0, 0, 0};
  down(cnt, d_cnt.get(), sizeof cnt);
  if (ok.ok() && stats)
    for (int c = 0; c < 4; ++c) stats[c] += (int64_t)cnt[c];
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}
