// script_core.h — scripted agents: the record an agent on a known track publishes, as plain functions that compile for the host form
// (script_host.cpp) AND for the device kernel (script_kernels.hip). One source, the same IEEE operations in the same order
// (floating-point contraction off, divisions correctly rounded on both sides), so the two forms agree bit for bit.
//
// Track. n_knots >= 1 knots (t, x, y, z), times in seconds, finite and strictly increasing. The state S(tau) = (p, v, a):
//   tau <= t_0                p_0, v = a = 0
//   tau >= t_last             p_last, v = a = 0
//   t_j <= tau < t_{j+1}      w = (p_{j+1} - p_j) / (t_{j+1} - t_j) (one division per axis), p = p_j + (tau - t_j) w, v = w, a = 0
// At an interior knot the RIGHT-hand segment's slope is the velocity.
//
// Record. In script round q (0 = the first round after the tracks were set) an agent publishes N + 1 states; state i has the time
// tau_i = (double)(q * step_plan + i) * dt — an integer product, one conversion, one rounding. State 0 is where the round starts,
// state step_plan where it ends (traj_curr of k_commit).
//   predict = 0   states[i] = S(tau_i) for every i: the prediction is the truth
//   predict = 1   states[i] = S(tau_i) for i <= step_plan; beyond it the state S(tau_sp) at i = step_plan goes on at constant
//                 velocity: p = p(tau_sp) + ((double)(i - step_plan) * dt) v(tau_sp), v = v(tau_sp), a = 0 — what an observer
//                 without the track would broadcast
// In both modes the first step_plan segments are the true motion: those are what the flight audit judges.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SCRIPT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SCRIPT_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_script {

constexpr int MAX_KNOTS = 256;

// S(tau) of the track knots[n_knots][4] into s[9] = (p, v, a)
SCRIPT_HD void track_state(const double* knots, int n_knots, double tau, double* s) {
  const double* last = knots + 4 * (size_t)(n_knots - 1);
  const double* a = knots;  // the knot the state rests at, or the left knot of the segment
  bool moving = false;
  if (tau <= knots[0]) {
  } else if (tau >= last[0]) {
    a = last;
  } else {
    int lo = 0, hi = n_knots - 1;  // t_lo <= tau < t_hi
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (knots[4 * (size_t)mid] <= tau) lo = mid;
      else hi = mid;
    }
    a = knots + 4 * (size_t)lo, moving = true;
  }
  s[0] = a[1], s[1] = a[2], s[2] = a[3];
  s[3] = s[4] = s[5] = s[6] = s[7] = s[8] = 0.0;
  if (moving) {
    const double* b = a + 4;
    const double span = b[0] - a[0], since = tau - a[0];
    const double wx = (b[1] - a[1]) / span, wy = (b[2] - a[2]) / span, wz = (b[3] - a[3]) / span;
    s[0] = a[1] + since * wx, s[1] = a[2] + since * wy, s[2] = a[3] + since * wz;
    s[3] = wx, s[4] = wy, s[5] = wz;
  }
}

SCRIPT_HD double state_time(long long round, int step_plan, int i, double dt) { return (double)(round * step_plan + i) * dt; }

// state i of the record of script round `round` into s[9]
SCRIPT_HD void record_state(const double* knots, int n_knots, int step_plan, double dt, int predict, long long round, int i, double* s) {
  const bool beyond = predict != 0 && i > step_plan;  // continued from the state the round ends in
  track_state(knots, n_knots, state_time(round, step_plan, beyond ? step_plan : i, dt), s);
  if (beyond) {
    const double ahead = (double)(i - step_plan) * dt;
    s[0] = s[0] + ahead * s[3], s[1] = s[1] + ahead * s[4], s[2] = s[2] + ahead * s[5];
  }
}

// tracks [n_script][n_knots][4] as hdsm_dswarm_set_script and hdsm_script_records_* accept them: 1 .. MAX_KNOTS knots, every entry
// finite, times strictly increasing
inline bool tracks_valid(int n_script, int n_knots, const double* knots) {
  if (n_knots < 1 || n_knots > MAX_KNOTS || n_script < 0 || (n_script > 0 && knots == nullptr)) return false;
  for (int k = 0; k < n_script; ++k)
    for (int j = 0; j < n_knots; ++j) {
      const double* e = knots + ((size_t)k * n_knots + j) * 4;
      for (int c = 0; c < 4; ++c)
        if (!std::isfinite(e[c])) return false;
      if (j > 0 && !(e[0] > e[-4])) return false;
    }
  return true;
}

}  // namespace hdsm_script
