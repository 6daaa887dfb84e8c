// mission_kernels.hip — missions (mission_core.h) on the device, for hdsm_mission_step_batch and the device-resident loop:
//   k_mission       one lane per flown agent, 64-lane workgroups. The lane steps its agent's record IN PLACE in global memory (a copy in
//                   registers would be indexed by the waypoint and land in scratch), writes the goal and the due flag of an agent that
//                   turns to another waypoint, and the wavefront adds its sums to the shard's tally: ballot / popcount for the three
//                   counts, a butterfly for the two 64-bit figures, ONE integer atomic per wavefront and field. No LDS, no scratch; an agent's record, goal and due flag have one owner.
//   k_mission_fold  one wavefront per neighbour group over the records of the group's local flown agents, 64 at a time (the pattern of
//                   k_group_report): integer sums, minima and maxima by butterflies. No LDS, no atomics.
// In the loop k_mission is the last launch of entry [5], behind k_vehicle; the arithmetic is mission_core.h's, the same source as the
// host forms.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/hdsm_swarm.h"
#include "device_mem.h"
#include "hdsm_internal.h"
#include "mission_core.h"
#include "mission_device.h"

namespace hdsm_mission_rule {
namespace {

__global__ __launch_bounds__(64) void k_mission(Launch a) {
  const int k = (int)(blockIdx.x * 64u + threadIdx.x);
  const bool active = k < a.n;
  int done = 0, stalled = 0, arrived = 0;
  long long total = 0, done_round = -1;
  if (active) {
    double s[6];
    const double* in = a.agents != nullptr ? a.agents[k].state_curr : a.states + (size_t)k * 9;
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = in[c];
    const double* wps = a.waypoints + (size_t)k * 3 * a.m.n_wp;
    hdsm_mission_record& r = a.records[k];
    double goal[3];
    int turn = 0;
    arrived = step(a.m, r, s, wps, a.count[k], a.round, goal, &turn);
    if (turn) {
      a.goals[3 * (size_t)k] = goal[0], a.goals[3 * (size_t)k + 1] = goal[1], a.goals[3 * (size_t)k + 2] = goal[2];
      a.due[k] = 1;
    }
    done = r.done, stalled = r.stalled != 0 && r.done == 0, total = r.arrivals, done_round = r.done_round;
  }
  // the wavefront's sums (every lane takes part; an idle lane holds the identities)
  const int n_done = __popcll(__ballot(done != 0)), n_stalled = __popcll(__ballot(stalled != 0)), n_arrived = __popcll(__ballot(arrived != 0));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    total += __shfl_xor(total, m, 64);
    const long long o = __shfl_xor(done_round, m, 64);
    done_round = o > done_round ? o : done_round;
  }
  if (threadIdx.x == 0) {
    Tally* t = a.tally + (a.round & 1);
    if (n_done) atomicAdd(&t->done, n_done);
    if (n_stalled) atomicAdd(&t->stalled, n_stalled);
    if (n_arrived) atomicAdd(&t->arrivals, n_arrived);
    if (total) atomicAdd(reinterpret_cast<unsigned long long*>(&t->arrivals_total), (unsigned long long)total);
    if (done_round >= 0) atomicMax(&t->done_round_max, done_round);
    if (blockIdx.x == 0) a.tally[(a.round + 1) & 1] = tally_identity();  // (nobody adds to the other slot in this launch)
  }
}

__global__ __launch_bounds__(64) void k_mission_fold(int first, int n_fly, const int32_t* __restrict__ gstart,
                                                     const hdsm_mission_record* __restrict__ records, hdsm_mission_group* __restrict__ out) {
  const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int lo = gstart[g], hi = gstart[g + 1];
  const int l0 = lo > first ? lo : first, l1 = hi < first + n_fly ? hi : first + n_fly;
  int done = 0, stalled = 0, laps_min = INT_MAX, laps_max = 0;
  long long arrivals = 0, makespan = -1;
  for (int a = l0 + lane; a < l1; a += 64) {
    const hdsm_mission_record& r = records[a - first];
    done += r.done, stalled += (r.stalled != 0 && r.done == 0), arrivals += r.arrivals;
    laps_min = r.laps < laps_min ? r.laps : laps_min, laps_max = r.laps > laps_max ? r.laps : laps_max;
    makespan = r.done_round > makespan ? r.done_round : makespan;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    done += __shfl_xor(done, m, 64), stalled += __shfl_xor(stalled, m, 64), arrivals += __shfl_xor(arrivals, m, 64);
    const int o_min = __shfl_xor(laps_min, m, 64), o_max = __shfl_xor(laps_max, m, 64);
    laps_min = o_min < laps_min ? o_min : laps_min, laps_max = o_max > laps_max ? o_max : laps_max;
    const long long o_mk = __shfl_xor(makespan, m, 64);
    makespan = o_mk > makespan ? o_mk : makespan;
  }
  if (lane == 0) {
    const int n = l1 > l0 ? l1 - l0 : 0;
    hdsm_mission_group r;
    r.first = lo, r.count = hi - lo, r.n_local = n, r.done = done;
    r.stalled = stalled, r.laps_min = n ? laps_min : 0, r.laps_max = laps_max, r.reserved0 = 0;
    r.arrivals = arrivals, r.makespan = done == n ? makespan : -1;
    out[g] = r;
  }
}

}  // namespace

hipError_t launch(const Launch& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mission, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fold(int n_groups, int first, int n_fly, const int32_t* gstart, const hdsm_mission_record* records, hdsm_mission_group* out,
                       hipStream_t st) {
  if (n_groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mission_fold, dim3((unsigned)n_groups), dim3(64), 0, st, first, n_fly, gstart, records, out);
  return hipGetLastError();
}

}  // namespace hdsm_mission_rule

extern "C" int hdsm_mission_step_batch(int32_t device, const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints,
                                       const int32_t* count, hdsm_mission_record* records, double* goals, uint8_t* due, hdsm_mission_summary* summary) {
  using namespace hdsm_mission_rule;
  const int rc = hdsm_internal_mission_args(m, n, round, states, waypoints, count, records, goals, due);
  if (rc) return rc;
  Tally tally[2] = {tally_identity(), tally_identity()};
  if (n > 0) {
    if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
    const size_t N = (size_t)n, W = N * 3 * (size_t)m->n_wp;
    hdsm_mem::DevBuf<double> d_states, d_wps, d_goals;
    hdsm_mem::DevBuf<int32_t> d_count;
    hdsm_mem::DevBuf<hdsm_mission_record> d_rec;
    hdsm_mem::DevBuf<uint8_t> d_due;
    hdsm_mem::DevBuf<Tally> d_tally;
    hdsm_mem::FirstError ok;
    ok(d_states.alloc(N * 9)), ok(d_wps.alloc(W)), ok(d_goals.alloc(N * 3)), ok(d_count.alloc(N)), ok(d_rec.alloc(N)), ok(d_due.alloc(N));
    ok(d_tally.alloc(2));
    if (ok.ok()) {
      ok(hipMemcpy(d_states.get(), states, N * 9 * sizeof(double), hipMemcpyHostToDevice));
      ok(hipMemcpy(d_wps.get(), waypoints, W * sizeof(double), hipMemcpyHostToDevice));
      ok(hipMemcpy(d_goals.get(), goals, N * 3 * sizeof(double), hipMemcpyHostToDevice));
      ok(hipMemcpy(d_count.get(), count, N * sizeof(int32_t), hipMemcpyHostToDevice));
      ok(hipMemcpy(d_rec.get(), records, N * sizeof(hdsm_mission_record), hipMemcpyHostToDevice));
      ok(hipMemcpy(d_due.get(), due, N, hipMemcpyHostToDevice));
      ok(hipMemcpy(d_tally.get(), tally, sizeof tally, hipMemcpyHostToDevice));
    }
    if (ok.ok()) {
      ok(launch(Launch{n, 0, (long long)round, *m, nullptr, d_states.get(), d_wps.get(), d_count.get(), d_rec.get(), d_goals.get(), d_due.get(),
                       d_tally.get()},
                nullptr));
      ok(hipDeviceSynchronize());
    }
    if (ok.ok()) {
      ok(hipMemcpy(records, d_rec.get(), N * sizeof(hdsm_mission_record), hipMemcpyDeviceToHost));
      ok(hipMemcpy(goals, d_goals.get(), N * 3 * sizeof(double), hipMemcpyDeviceToHost));
      ok(hipMemcpy(due, d_due.get(), N, hipMemcpyDeviceToHost));
      ok(hipMemcpy(tally, d_tally.get(), sizeof tally, hipMemcpyDeviceToHost));
    }
    if (!ok.ok()) return HDSM_ERR_DEVICE;
  }
  if (summary) *summary = summary_of(tally[round & 1], round, n);
  return HDSM_OK;
}
