// mission_core.h — missions: per agent a list of waypoints visited in order, arrival, stalls and the shard's summary, as plain
// functions that compile for the host forms (mission_host.cpp, swarm_models.cpp) AND for the device kernel (mission_kernels.hip). One
// source, the same IEEE operations in the same order (floating-point contraction off, products first, sums left to right, sqrt
// correctly rounded on both sides), so the forms agree bit for bit. The rule is written out in include/hdsm_swarm.h ("missions"); the
// order of the statements of step() IS its definition.
//
// A record is stepped IN PLACE (in global memory on the device): arrive_round is indexed by the waypoint, and a copy in registers
// would put the kernel on scratch memory.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/hdsm_swarm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISSION_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MISSION_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

static_assert(sizeof(hdsm_mission) == 48, "hdsm_mission is 48 bytes");
static_assert(sizeof(hdsm_mission_record) == 128, "hdsm_mission_record is 128 bytes");
static_assert(sizeof(hdsm_mission_summary) == 40, "hdsm_mission_summary is 40 bytes");
static_assert(sizeof(hdsm_mission_group) == 48, "hdsm_mission_group is 48 bytes");

namespace hdsm_mission_rule {

constexpr int MAX_WP = HDSM_MISSION_MAX_WP;

// the squared distance of p[3] to w[3], and whether a sum of squares is a finite number (false for an infinity and a NaN, without libm)
MISSION_HD double dist2(const double* p, const double* w) {
  const double dx = p[0] - w[0], dy = p[1] - w[1], dz = p[2] - w[2];
  return (dx * dx + dy * dy) + dz * dz;
}
MISSION_HD bool finite1(double x) { return x - x == 0.0; }

// best_dist of an agent that turns to waypoint w from the state s
MISSION_HD double leg_length(const double* s, const double* w) {
  const double d2 = dist2(s, w);
  return finite1(d2) ? sqrt(d2) : DBL_MAX;
}

// the record of an agent at the start of a mission: no distance seen yet, so the first round judged counts as progress
inline void reset(hdsm_mission_record& r) {
  r.wp = r.done = r.dwell = r.stalled = 0;
  r.laps = r.stall_events = r.since = r.arrivals = 0;
  r.done_round = -1, r.last_arrival_round = -1;
  r.dist = 0.0, r.best_dist = DBL_MAX;
  for (int i = 0; i < MAX_WP; ++i) r.arrive_round[i] = -1;
}

// One step of one agent in mission round m: s[9] its state as the round leaves it, wps [n_wp][3] its waypoints, count of them in
// use. Returns 1 for an arrival; *turn = 1 when the agent turns to another waypoint (goal[3] = that waypoint, the agent is due).
MISSION_HD int step(const hdsm_mission& m, hdsm_mission_record& r, const double* s, const double* wps, int count, long long round, double* goal,
                    int* turn) {
  *turn = 0;
  if (r.done) return 0;
  const double* w = wps + 3 * (size_t)r.wp;
  const double d2 = dist2(s, w), d = sqrt(d2);
  const double v2 = (s[3] * s[3] + s[4] * s[4]) + s[5] * s[5];
  const double R = m.arrive_radius, V = m.arrive_speed;
  const bool finite = finite1(d2) && finite1(v2);
  const bool inside = finite && d2 <= R * R && (V <= 0.0 || v2 <= V * V);
  r.dist = finite ? d : -1.0;
  r.dwell = inside ? r.dwell + 1 : 0;
  if (r.dwell >= m.dwell_rounds) {
    r.arrive_round[r.wp] = (int32_t)round, r.last_arrival_round = round;
    r.arrivals += 1, r.wp += 1, r.dwell = 0;
    if (r.wp == count) {
      if (m.loop) r.wp = 0, r.laps += 1;
      else r.done = 1, r.done_round = round;
    }
    if (!r.done) {
      const double* nw = wps + 3 * (size_t)r.wp;
      goal[0] = nw[0], goal[1] = nw[1], goal[2] = nw[2];
      *turn = 1;
      r.best_dist = leg_length(s, nw), r.since = 0, r.stalled = 0;
    }
    return 1;
  }
  if (finite && d < r.best_dist - m.stall_eps) {
    r.best_dist = d, r.since = 0, r.stalled = 0;
  } else {
    r.since += 1;
    if (m.stall_rounds > 0 && r.since == m.stall_rounds) r.stalled = 1, r.stall_events += 1;
  }
  return 0;
}

// the running figures of a shard's summary: integer sums and a maximum (its identity: -1)
struct Tally {
  int32_t done, stalled, arrivals, pad;
  long long arrivals_total, done_round_max;
};
MISSION_HD Tally tally_identity() { return Tally{0, 0, 0, 0, 0, -1}; }
inline void tally_add(Tally& t, const hdsm_mission_record& r, int arrived) {
  t.done += r.done, t.stalled += (r.stalled != 0 && r.done == 0), t.arrivals += arrived, t.arrivals_total += r.arrivals;  // (stalled NOW: not a done agent)
  if (r.done_round > t.done_round_max) t.done_round_max = r.done_round;
}
inline hdsm_mission_summary summary_of(const Tally& t, long long round, int flown) {
  hdsm_mission_summary s;
  s.round = round, s.flown = flown, s.done = t.done, s.stalled = t.stalled, s.arrivals = t.arrivals, s.arrivals_total = t.arrivals_total;
  s.makespan = t.done == flown ? t.done_round_max : -1;
  return s;
}

// a setting with its table as hdsm_*_set_mission and hdsm_mission_step_* accept it (n agents)
inline bool setting_valid(const hdsm_mission* m, int n, const double* waypoints, const int32_t* count) {
  if (m == nullptr || m->n_wp < 1 || m->n_wp > MAX_WP || (m->loop != 0 && m->loop != 1) || m->dwell_rounds < 1 || m->stall_rounds < 0) return false;
  if (!std::isfinite(m->arrive_radius) || !(m->arrive_radius > 0) || !std::isfinite(m->arrive_speed) || !std::isfinite(m->stall_eps) || m->stall_eps < 0)
    return false;
  if (n < 0 || (n > 0 && (waypoints == nullptr || count == nullptr))) return false;
  for (int k = 0; k < n; ++k) {
    if (count[k] < 1 || count[k] > m->n_wp) return false;
    for (int e = 0; e < 3 * m->n_wp; ++e)
      if (!std::isfinite(waypoints[(size_t)k * 3 * m->n_wp + e])) return false;
  }
  return true;
}

}  // namespace hdsm_mission_rule
