// mission_device.h — the launch interface of k_mission and k_mission_fold (mission_kernels.hip), used by hdsm_mission_step_batch and by
// the device-resident loop (the round: swarm_kernels.hip; set-up, groups and downloads: dswarm_models.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "mission_core.h"
#include "swarm_core.h"

namespace hdsm_mission_rule {

// One launch over n agents, one lane each. The state of agent k is agents[k].state_curr (the loop) or states [n][9] (the batch).
// One step in mission round `round`: records in place, goals / due of the agents that turn to another waypoint, and the shard's sums
// into tally[round & 1] — one atomic per wavefront and field — while tally[(round + 1) & 1] is set to the identity for the next
// round (both slots hold the identity before the first round).
struct Launch {
  int32_t n, pad;
  long long round;
  hdsm_mission m;
  const hdsm_sw::AgentS* agents;
  const double* states;
  const double* waypoints;  // [n][m.n_wp][3]
  const int32_t* count;     // [n]
  hdsm_mission_record* records;
  double* goals;  // [n][3]
  uint8_t* due;   // [n]
  Tally* tally;   // [2]
};
hipError_t launch(const Launch& a, hipStream_t st);  // (nothing is launched for n == 0)

// One wavefront per group g over the records of its local flown agents [max(gstart[g], first), min(gstart[g + 1], first + n_fly)).
hipError_t launch_fold(int n_groups, int first, int n_fly, const int32_t* gstart, const hdsm_mission_record* records, hdsm_mission_group* out,
                       hipStream_t st);

}  // namespace hdsm_mission_rule
