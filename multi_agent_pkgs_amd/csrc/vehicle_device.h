// vehicle_device.h — the launch interface of k_vehicle and k_seat (vehicle_kernels.hip), used by hdsm_vehicle_fly_batch and by the
// device-resident loop (the round: swarm_kernels.hip, right behind k_command; the seating: dswarm_models.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "swarm_core.h"
#include "vehicle_core.h"

namespace hdsm_veh {

// One launch over n agents, one lane each. Two forms, told apart by `agents`:
//   loop    agents [n] as k_commit left them + records [n]: knot 0 is traj_curr[0], planned_end is state_curr, which takes the flown
//           state; the sample is booked in the agent's track record; the id is the agent's
//   batch   no agents: ids [n], start [n][9], planned_end [n][9] -> flown [n][9], dist [n] (or NULL)
// Both: setpoint [n][step_plan], vstate [n] in and out, pose [n] (or NULL), cnt[4] += agent-rounds flown, reseated,
// sub-steps with the thrust clamped, with a rate clamped (atomics: one add per wavefront and counter).
struct Launch {
  int32_t n, step_plan;
  long long q;
  double dt;
  hdsm_vehicle m;
  hdsm_sw::AgentS* agents;
  hdsm_track_record* records;
  const int32_t* ids;
  const double* start;
  const double* planned_end;
  double* flown;
  double* dist;
  const hdsm_command* setpoint;
  hdsm_vehicle_state* vstate;
  hdsm_command* pose;
  unsigned long long* cnt;
};
hipError_t launch(const Launch& a, hipStream_t st);  // (nothing is launched for n == 0)

// k_seat: vstate[k] = seat(row k of states, yaw[k]) for k < n where mask (or NULL: all) is set and the row is finite. Row k starts
// stride doubles behind row k - 1 (9: a plain array; sizeof(AgentS) / 8 from &agents[0].state_curr[0]: the agents' own states).
struct Seat {
  int32_t n;
  hdsm_vehicle m;
  const double* states;
  size_t stride;
  const double* yaw;
  const uint8_t* mask;
  hdsm_vehicle_state* vstate;
};
hipError_t launch_seat(const Seat& a, hipStream_t st);

}  // namespace hdsm_veh
