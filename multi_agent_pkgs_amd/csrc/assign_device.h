// assign_device.h — the launch interface of k_assign (assign_kernels.hip), used by hdsm_assign_batch and by hdsm_dswarm_assign
// (dswarm_models.cpp), and the argument checks the host form shares with them (assign_host.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "assign_core.h"
#include "swarm_core.h"

namespace hdsm_assign {

// One launch, one workgroup per group. The position of agent k is agents[k].state_curr (the loop) or pos [n][3] (the batch); agent k
// is active when k < n_on and (active == NULL or active[k] != 0). gstart [n_groups + 1] on the device. slot_of [n], price [n] (may be
// NULL) and stats [n_groups] are written whole: first and count of a group's stats too.
struct Launch {
  Rule rule;
  int32_t n_groups, n_on;
  const int32_t* gstart;
  const hdsm_sw::AgentS* agents;
  const double* pos;
  const uint8_t* active;
  const double* slots;
  int32_t* slot_of;
  int64_t* price;
  hdsm_assign_stats* stats;
};
// m_max: the largest number of active agents of a group, 0 .. MAX_M (the workgroup has that many threads, rounded up to wavefronts).
// Nothing is launched for n_groups == 0.
hipError_t launch(const Launch& a, int m_max, hipStream_t st);

}  // namespace hdsm_assign
