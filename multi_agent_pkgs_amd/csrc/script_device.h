// script_device.h — the launch interface of k_script (script_kernels.hip), used by hdsm_script_records_batch and by the
// device-resident loop (swarm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "script_core.h"
#include "swarm_core.h"

namespace hdsm_script {

// One script round of n_script agents: knots [n_script][n_knots][4] and records [n_script][N + 1][9] on the device. The loop also
// gives the slots' flags, statuses and agent states (each [n_script], the scripted tail of its array); the batch form leaves the
// three NULL and gets the records alone.
struct Round {
  int32_t n_script, n_knots, N, step_plan, predict;
  long long round;
  double dt;
  const double* knots;
  double* records;
  uint8_t* has;
  int32_t* status;
  hdsm_sw::AgentS* agents;
};
hipError_t launch(const Round& r, hipStream_t st);  // (nothing is launched for n_script == 0)

}  // namespace hdsm_script
