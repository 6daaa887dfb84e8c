// dswarm_audit.hip — what the device-resident loop reports about a flight between its rounds: the flight audit and the state history
// (switched here; launched by the round, swarm_kernels.hip audit_and_history, through audit_device.h) and the per-group summary
// (k_group_report, launched here and nowhere else).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <vector>

#include "dswarm.h"
#include "hdsm_internal.h"

using namespace hdsm_dswarm;

namespace {

// ---- neighbour groups: the per-group flight summary (hdsm_dswarm_group_report) ----
// One wavefront per group over the group's LOCAL agents [max(lo, first), min(hi, first + n_local)), 64 at a time; groups larger than
// a wavefront loop. Every figure is an integer sum, a minimum or a maximum, reduced over the wave by butterflies: the result does not
// depend on the order. The separation minimum orders (sep2_min, agent id) — a total order: ties go to the lower agent id. No atomics,
// no LDS. report == nullptr (the audit was never on): the audit fields are zeros and -1. With the audit on, a group without a pair
// (one agent) has sep2_min = DBL_MAX and sep_agent = -1, as in an empty hdsm_flight_report.
template <class T>
__device__ __forceinline__ T wave_xor(T v, int m) {
  return __shfl_xor(v, m, 64);
}
__global__ __launch_bounds__(64) void k_group_report(int first, int n_local, const int32_t* __restrict__ gstart, const AgentS* __restrict__ agents,
                                                     const int32_t* __restrict__ status, const hdsm_flight_report* __restrict__ report,
                                                     hdsm_group_report* __restrict__ out) {
  const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int lo = gstart[g], hi = gstart[g + 1];
  const int l0 = lo > first ? lo : first, l1 = hi < first + n_local ? hi : first + n_local;
  long long no_sol = 0, failed = 0, rounds = 0, positions = 0, close_r = 0, occupied = 0, unknown = 0, crossed = 0, pot = 0;
  double dist_goal = 0.0, speed_max = 0.0, q = DBL_MAX;
  int q_agent = -1, q_partner = -1, q_sub = 0;
  long long q_round = -1;
  for (int a = l0 + lane; a < l1; a += 64) {
    const int k = a - first;
    const AgentS& ag = agents[k];
    no_sol += status[k] == HDSM_NO_SOLUTION, failed += ag.n_fail;
    const double dg = hdsm_sw::norm(hdsm_sw::sub(V3{{ag.state_curr[0], ag.state_curr[1], ag.state_curr[2]}}, ag.goal));
    dist_goal = dg > dist_goal ? dg : dist_goal;
    if (report != nullptr) {
      const hdsm_flight_report r = report[k];
      rounds = r.rounds > rounds ? r.rounds : rounds;
      positions += r.positions, close_r += r.close_rounds, occupied += r.occupied, unknown += r.unknown, crossed += r.crossed, pot += r.pot_sum;
      speed_max = r.speed_max > speed_max ? r.speed_max : speed_max;
      if (r.sep_partner >= 0 && (q_agent < 0 || r.sep2_min < q))  // (ids ascend within a lane: '<' keeps the lower one)
        q = r.sep2_min, q_agent = a, q_partner = r.sep_partner, q_sub = r.sep_substep, q_round = r.sep_round;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    no_sol += wave_xor(no_sol, m), failed += wave_xor(failed, m), positions += wave_xor(positions, m), close_r += wave_xor(close_r, m);
    occupied += wave_xor(occupied, m), unknown += wave_xor(unknown, m), crossed += wave_xor(crossed, m), pot += wave_xor(pot, m);
    const long long o_rounds = wave_xor(rounds, m);
    rounds = o_rounds > rounds ? o_rounds : rounds;
    const double o_dg = wave_xor(dist_goal, m), o_sp = wave_xor(speed_max, m);
    dist_goal = o_dg > dist_goal ? o_dg : dist_goal, speed_max = o_sp > speed_max ? o_sp : speed_max;
    const double o_q = wave_xor(q, m);
    const int o_agent = wave_xor(q_agent, m), o_partner = wave_xor(q_partner, m), o_sub = wave_xor(q_sub, m);
    const long long o_round = wave_xor(q_round, m);
    if (o_agent >= 0 && (q_agent < 0 || o_q < q || (o_q == q && o_agent < q_agent)))
      q = o_q, q_agent = o_agent, q_partner = o_partner, q_sub = o_sub, q_round = o_round;
  }
  if (lane == 0) {
    hdsm_group_report r;
    r.first = lo, r.count = hi - lo, r.n_local = l1 > l0 ? l1 - l0 : 0, r.no_solution_last = (int32_t)no_sol;
    r.failed_total = failed, r.dist_goal_max = dist_goal;
    r.rounds = rounds, r.positions = positions, r.close_rounds = close_r, r.occupied = occupied, r.unknown = unknown, r.crossed = crossed;
    r.pot_sum = pot, r.sep2_min = report != nullptr ? q : 0.0, r.sep_agent = q_agent, r.sep_partner = q_partner, r.sep_substep = q_sub, r.reserved0 = 0;
    r.sep_round = q_round, r.speed_max = speed_max;
    out[g] = r;
  }
}

}  // namespace

// the audit's scratch and (at the first switch-on) the flight record of the shard; `init` [n_local] or empty reports
int hdsm_dswarm::audit_setup(DSwarm* d, const hdsm_flight_report* init) {
  Audit& a = d->audit;
  if (!a.buf.d_round) {
    if (hdsm_audit::device_alloc(&a.buf, d->slots(), d->n_local, d->c.step_plan) != hipSuccess)
      return fail(HDSM_ERR_DEVICE, "flight audit: allocation failed");
  }
  if (!a.d_report && (init != nullptr || a.on)) {
    std::vector<hdsm_flight_report> rep((size_t)d->n_local);
    for (int k = 0; k < d->n_local; ++k) {
      if (init) rep[k] = init[k];
      else hdsm_audit::empty_report(&rep[k]);
    }
    HIP_TRY(a.d_report.alloc(rep.size() + 1));
    if (!rep.empty()) HIP_TRY(hipMemcpy(a.d_report.get(), rep.data(), rep.size() * sizeof(hdsm_flight_report), hipMemcpyHostToDevice));
    a.ever = true;
  }
  return HDSM_OK;
}

extern "C" {

// The flight per group (one record for the whole swarm without a partition): k_group_report over the agents' states, the last
// statuses and — once the audit has been on — the flight records. Launched here and nowhere else: a round never pays for it.
int hdsm_dswarm_group_report(void* dswarm, hdsm_group_report* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  const int ng = (int)d->group_start.size() - 1;
  if (int rc = device_idle(d)) return rc;
  if (!d->d_gstart) {
    HIP_TRY(d->d_gstart.alloc(d->group_start.size()));
    HIP_TRY(hipMemcpy(d->d_gstart.get(), d->group_start.data(), d->group_start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(d->d_greport.alloc((size_t)ng));
  }
  hipLaunchKernelGGL(k_group_report, dim3((unsigned)ng), dim3(64), 0, nullptr, d->first, d->n_local, d->d_gstart.get(), d->d_agents.get(), d->d_status.get(),
                     d->audit.ever ? d->audit.d_report.get() : nullptr, d->d_greport.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d->d_greport.get(), (size_t)ng * sizeof(hdsm_group_report), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// ---- the flight audit and the state history of the device loop (audit_kernels.hip) ----
int hdsm_dswarm_set_audit(void* dswarm, int32_t on, double sep_warn) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (!(sep_warn > 0)) return fail(HDSM_ERR_BAD_ARG, "sep_warn must be positive");
  if (int rc = device_idle(d)) return rc;
  d->audit.on = on != 0, d->audit.sep_warn = sep_warn;
  if (on) {
    if (int rc = audit_setup(d, nullptr)) return rc;
    if (d->phase_timing)
      if (int rc = timing_events(d)) return rc;
  }
  return HDSM_OK;
}

int hdsm_dswarm_flight_report(void* dswarm, hdsm_flight_report* report) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (d->n_local && !report)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->audit.ever) return fail(HDSM_ERR_BAD_ARG, "the flight audit was never switched on");
  if (int rc = device_idle(d)) return rc;
  if (d->n_local) HIP_TRY(hipMemcpy(report, d->audit.d_report.get(), (size_t)d->n_local * sizeof(hdsm_flight_report), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_last_audit_round(void* dswarm, hdsm_audit_round* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (d->n_local && !out)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->audit.on || d->audit.rounds == 0) return fail(HDSM_ERR_BAD_ARG, "no round has been audited (hdsm_dswarm_set_audit)");
  if (int rc = device_idle(d)) return rc;
  if (d->n_local) HIP_TRY(hipMemcpy(out, d->audit.buf.d_round.get(), (size_t)d->n_local * sizeof(hdsm_audit_round), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// The audit's launches of the last timed round (pack, sweep, track; or the history write alone), in milliseconds; 0 when that round
// launched none or no round was timed. Kept out of hdsm_dswarm_last_phase_ms: the audit starts after its [6].
int hdsm_dswarm_last_audit_ms(void* dswarm, float* ms) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !ms) return fail(HDSM_ERR_BAD_ARG, "null argument");
  *ms = 0.0f;
  if (!d->audit.timed.valid) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(d->audit.timed.ms(ms));
  return HDSM_OK;
}

int hdsm_dswarm_set_history(void* dswarm, int32_t capacity_rounds) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || capacity_rounds < 0) return fail(HDSM_ERR_BAD_ARG, "bad argument");
  if (int rc = device_idle(d)) return rc;
  History& h = d->hist;
  h.d_rows.reset();
  h.cap = 0, h.n = h.dropped = h.delivered = 0, h.last = false;
  if (capacity_rounds > 0) {
    if (int rc = audit_setup(d, nullptr)) return rc;
    HIP_TRY(h.d_rows.alloc((size_t)capacity_rounds * d->n_local * 9 + 1));
    h.cap = capacity_rounds;
    if (d->phase_timing)
      if (int rc = timing_events(d)) return rc;
  }
  return HDSM_OK;
}

int hdsm_dswarm_download_history(void* dswarm, void* swarm, double* hist, int32_t max_rounds, int32_t* n_rounds, int32_t* dropped) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || max_rounds < 0 || (hist == nullptr && max_rounds > 0)) return fail(HDSM_ERR_BAD_ARG, "bad argument");
  History& h = d->hist;
  if (h.cap == 0) return fail(HDSM_ERR_BAD_ARG, "the history is off (hdsm_dswarm_set_history)");
  if (int rc = device_idle(d)) return rc;
  const size_t row = (size_t)d->n_local * 9;
  const int n_copy = h.n < max_rounds ? h.n : max_rounds;
  if (n_copy > 0 && row) HIP_TRY(hipMemcpy(hist, h.d_rows.get(), (size_t)n_copy * row * sizeof(double), hipMemcpyDeviceToHost));
  if (swarm && h.n > h.delivered) {  // every recorded round reaches the mirror's planner records once
    const int m = h.n - h.delivered;
    std::vector<double> rows((size_t)m * row);
    if (row) HIP_TRY(hipMemcpy(rows.data(), h.d_rows.get() + (size_t)h.delivered * row, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int rc = hdsm_swarm_append_history(swarm, m, rows.data());
    if (rc) return fail(rc, "hdsm_swarm_append_history");
    h.delivered = h.n;
  }
  if (n_rounds) *n_rounds = h.n;
  if (dropped) *dropped = h.dropped;
  return HDSM_OK;
}

}  // extern "C"
