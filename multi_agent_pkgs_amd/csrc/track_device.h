// track_device.h — the launch interface of k_track (track_kernels.hip), used by hdsm_track_states_batch and by the device-resident
// loop (the model form: swarm_kernels.hip; the external form: dswarm_models.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "swarm_core.h"
#include "track_core.h"

namespace hdsm_track {

// One launch over n agents, one lane each. Three forms, told apart by the pointers that are set:
//   model      agents + records: state_curr = the flown state of traj_curr[step_plan] in tracking round q, for the agents that have a plan
//   external   agents + records + src [n][9] (+ mask [n] or NULL: all): state_curr = the supplied row where it is masked and finite,
//              and with it the agent's entry of hist_row
//   batch      ids + planned + flown (+ dist or NULL), no agents: hdsm_track_states_batch
struct Launch {
  int32_t n, step_plan;
  long long q;
  double T;
  hdsm_tracking model;
  hdsm_sw::AgentS* agents;
  hdsm_track_record* records;
  const double* src;
  const uint8_t* mask;
  const int32_t* ids;
  const double* planned;
  double* flown;
  double* dist;
  double* hist_row;  // (external form, or NULL) the history row [n][9] of the round the states were measured behind
};
hipError_t launch(const Launch& a, hipStream_t st);  // (nothing is launched for n == 0)

}  // namespace hdsm_track
