// command_device.h — the launch interface of k_command (command_kernels.hip), used by hdsm_command_batch and by the device-resident
// loop (swarm_kernels.hip, right behind k_commit / k_track / k_script).
#pragma once
#include <hip/hip_runtime.h>

#include "command_core.h"
#include "swarm_core.h"

namespace hdsm_cmd {

// One launch over n agents, one lane each. Two forms, told apart by `agents`:
//   loop    agents [n] as k_commit (and k_track) left them + status [n_fly]: the record is traj_curr, the state after state_curr, valid
//           from status and has_traj; before = the solver's x_0 input [n_fly][9] (state_curr of before the commit), ref_full [n_fly][N + 1][6]
//           this round's reference (n_ref = N + 1). Lanes n_fly .. n - 1 (the scripted tail) write zeros.
//   batch   no agents: n_ref [n], ref_point [n][3], before [n][9], records [n][N + 1][9], valid_in [n], after [n][9]
// Both: yaw [n] in and out, setpoint [n][step_plan], pose [n] (either NULL in the batch form), cnt[2] += steps taken, skipped (atomics: one
// add per wavefront and counter).
struct Launch {
  int32_t n, n_fly, N, step_plan, yaw_idx, pad;
  double dt, k_p_yaw;
  const hdsm_sw::AgentS* agents;
  const int32_t* status;
  const double* before;
  const double* ref_full;
  const int32_t* n_ref;
  const double* ref_point;
  const double* records;
  const int32_t* valid_in;
  const double* after;
  double* yaw;
  hdsm_command* setpoint;
  hdsm_command* pose;
  unsigned long long* cnt;
};
hipError_t launch(const Launch& a, hipStream_t st);  // (nothing is launched for n == 0)

}  // namespace hdsm_cmd
