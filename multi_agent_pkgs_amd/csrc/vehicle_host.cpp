// vehicle_host.cpp — the host forms of a vehicle in the loop (vehicle_core.h): hdsm_vehicle_default, hdsm_vehicle_seat_host,
// hdsm_vehicle_fly_host and the argument checks the last shares with hdsm_vehicle_fly_batch. Pure host C++; the device form
// (vehicle_kernels.hip) gives the same bits.
#include <cmath>

#include "../../include/hdsm.h"
#include "../../include/hdsm_swarm.h"
#include "hdsm_internal.h"
#include "vehicle_core.h"

static_assert(sizeof(hdsm_vehicle_state) == 128, "hdsm_vehicle_state is a 128-byte record");
static_assert(sizeof(hdsm_vehicle) == 224, "hdsm_vehicle is 224 bytes");

extern "C" int hdsm_internal_vehicle_args(const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt, int64_t round,
                                          const double* start, const hdsm_command* setpoint, const double* planned_end,
                                          const hdsm_vehicle_state* vstate, const double* flown) {
  if (!hdsm_veh::settings_valid(m) || n < 0 || step_plan < 1 || step_plan > HDSM_MAX_HOR) return HDSM_ERR_BAD_ARG;
  if (n > 0 && (!agent_id || !start || !setpoint || !planned_end || !vstate || !flown)) return HDSM_ERR_BAD_ARG;
  if (!std::isfinite(dt) || !(dt > 0)) return HDSM_ERR_BAD_ARG;
  if (round < 0 || round > hdsm_track::MAX_ROUND) return HDSM_ERR_BAD_ARG;
  return HDSM_OK;
}

// A Crazyflie-class setting. PROPOSALS: no flight was measured with them. A 27 g vehicle with a thrust-to-weight ratio near 1.9
// (thrust_max 18 m/s^2), outer-loop gains for a natural frequency of about 2.6 rad/s at a damping ratio near 1, an attitude loop
// (k_att 12 / s behind a 30 ms rate lag) a decade faster, body rates limited to 10 rad/s in roll and pitch and 4 rad/s in yaw, a
// 50 ms thrust lag, a light linear drag. They are chosen so that a 1 m step under the hold feed settles to 1 % within 5 s without
// ever leaving the step's range (tests/test_vehicle.py) — a condition on the numbers, not a measurement of a vehicle.
extern "C" int hdsm_vehicle_default(hdsm_vehicle* m) {
  if (!m) return HDSM_ERR_BAD_ARG;
  *m = hdsm_vehicle{};
  m->n_sub = 10, m->feed = 0, m->acc_from = 0;
  for (int k = 0; k < 3; ++k) {
    m->kp[k] = k == 2 ? 10.0 : 7.0, m->kv[k] = k == 2 ? 6.0 : 5.0, m->k_att[k] = k == 2 ? 4.0 : 12.0;
    m->rate_max[k] = k == 2 ? 4.0 : 10.0, m->drag[k] = 0.1;
  }
  m->tau_rate = 0.03, m->tau_thrust = 0.05, m->thrust_min = 2.0, m->thrust_max = 18.0;
  return HDSM_OK;
}

extern "C" int hdsm_vehicle_seat_host(const hdsm_vehicle* m, int32_t n, const double* states, const double* yaw, hdsm_vehicle_state* out) {
  if (!hdsm_veh::settings_valid(m) || n < 0 || (n > 0 && (!states || !yaw || !out))) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < n; ++k) hdsm_veh::seat(*m, states + (size_t)k * 9, yaw[k], out[k]);
  return HDSM_OK;
}

extern "C" int hdsm_vehicle_fly_host(const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt, int64_t round,
                                     const double* start, const hdsm_command* setpoint, const double* planned_end, hdsm_vehicle_state* vstate,
                                     double* flown, double* dist, hdsm_command* pose, int64_t stats[4]) {
  const int rc = hdsm_internal_vehicle_args(m, n, agent_id, step_plan, dt, round, start, setpoint, planned_end, vstate, flown);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    double s0[9], pe[9], out[9], d, dvel;  // (planned_end and flown may be the same array)
    for (int c = 0; c < 9; ++c) s0[c] = start[(size_t)k * 9 + c], pe[c] = planned_end[(size_t)k * 9 + c];
    int n_thrust = 0, n_rate = 0;
    const int ok = hdsm_veh::agent_round(*m, agent_id[k], round, step_plan, dt, s0, setpoint + (size_t)k * step_plan, pe, vstate[k], out, &d, &dvel,
                                         pose ? pose + k : nullptr, &n_thrust, &n_rate);
    for (int c = 0; c < 9; ++c) flown[(size_t)k * 9 + c] = out[c];
    if (dist) dist[k] = d;
    if (stats) stats[0] += ok, stats[1] += 1 - ok, stats[2] += n_thrust, stats[3] += n_rate;
  }
  return HDSM_OK;
}
