// mission_host.cpp — the host form of a mission step (mission_core.h): hdsm_mission_step_host and the argument checks it shares with
// hdsm_mission_step_batch. Pure host C++; the device form (mission_kernels.hip) gives the same bits.
#include "../../include/hdsm_swarm.h"
#include "hdsm_internal.h"
#include "mission_core.h"

extern "C" int hdsm_internal_mission_args(const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints,
                                          const int32_t* count, const hdsm_mission_record* records, const double* goals, const uint8_t* due) {
  if (round < 0 || !hdsm_mission_rule::setting_valid(m, n, waypoints, count)) return HDSM_ERR_BAD_ARG;
  if (n > 0 && (!states || !records || !goals || !due)) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < n; ++k)
    if (records[k].wp < 0 || records[k].wp >= count[k] + (records[k].done != 0)) return HDSM_ERR_BAD_ARG;  // (a done record stands behind its last)
  return HDSM_OK;
}

extern "C" int hdsm_mission_step_host(const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints,
                                      const int32_t* count, hdsm_mission_record* records, double* goals, uint8_t* due, hdsm_mission_summary* summary) {
  const int rc = hdsm_internal_mission_args(m, n, round, states, waypoints, count, records, goals, due);
  if (rc) return rc;
  hdsm_mission_rule::Tally t = hdsm_mission_rule::tally_identity();
  for (int k = 0; k < n; ++k) {
    double goal[3];
    int turn = 0;
    const int arrived =
        hdsm_mission_rule::step(*m, records[k], states + (size_t)k * 9, waypoints + (size_t)k * 3 * m->n_wp, count[k], round, goal, &turn);
    if (turn) {
      for (int c = 0; c < 3; ++c) goals[3 * (size_t)k + c] = goal[c];
      due[k] = 1;
    }
    hdsm_mission_rule::tally_add(t, records[k], arrived);
  }
  if (summary) *summary = hdsm_mission_rule::summary_of(t, round, n);
  return HDSM_OK;
}
