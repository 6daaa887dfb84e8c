// dswarm_assign.cpp — formations in the device-resident loop: hdsm_dswarm_assign runs k_assign (assign_kernels.hip, through
// assign_device.h) on the agents' state_curr where it lives; only slot_of and the stats come back. A set-up call between rounds, launched
// here and nowhere else: a round never pays for it. apply = 1 hands the permuted slots to hdsm_dswarm_set_goals.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "assign_device.h"
#include "dswarm.h"

using namespace hdsm_dswarm;

extern "C" int hdsm_dswarm_assign(void* dswarm, const hdsm_assign_setting* setting, const double* slots, int32_t apply, int32_t* slot_of,
                                  hdsm_assign_stats* stats) {
  using namespace hdsm_assign;
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (apply != 0 && apply != 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_assign: apply is 0 or 1");
  if (d->world != 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_assign: world_size 1 only (a group's agents must all be local)");
  if (apply && d->mission.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_assign: a mission is on (hdsm_dswarm_set_mission): the goals are its waypoints");
  const int n = d->n_local, ng = (int)d->group_start.size() - 1;
  Assign& as = d->assign;
  std::vector<int32_t> gs, own((size_t)n);
  Rule rule;
  int m_max = 0;
  const int rc = check_args(setting, n, d->grouped ? ng : 0, d->grouped ? d->group_start.data() : nullptr, true, nullptr, d->n_fly(), slots, own.data(),
                            &rule, &gs, &m_max);
  if (rc == HDSM_ERR_CAPACITY) return fail(rc, "hdsm_dswarm_assign: a group of more than HDSM_ASSIGN_MAX flown agents");
  if (rc) return fail(rc, "hdsm_dswarm_assign: a null argument, a slot that is not finite or a setting out of its bounds (include/hdsm_swarm.h)");
  const size_t G = gs.size() - 1;
  std::vector<hdsm_assign_stats> st(G);
  if (n > 0) {
    if (int rd = device_idle(d)) return rd;
    if (!as.ready()) {
      hdsm_mem::FirstError ok;
      ok(as.d_slots.alloc((size_t)n * 3)), ok(as.d_slot_of.alloc((size_t)n)), ok(as.d_gstart.alloc(gs.size())), ok(as.d_stats.alloc(G));
      if (ok.ok()) ok(hipMemcpy(as.d_gstart.get(), gs.data(), gs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      if (!ok.ok()) {
        as.d_stats.reset();
        return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_assign: ") + hipGetErrorString(ok.e));
      }
    }
    HIP_TRY(hipMemcpy(as.d_slots.get(), slots, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch(Launch{rule, (int32_t)G, d->n_fly(), as.d_gstart.get(), d->d_agents.get(), nullptr, nullptr, as.d_slots.get(), as.d_slot_of.get(), nullptr,
                          as.d_stats.get()},
                   m_max, nullptr));
    as.launches += 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(own.data(), as.d_slot_of.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st.data(), as.d_stats.get(), G * sizeof(hdsm_assign_stats), hipMemcpyDeviceToHost));
  } else {
    st[0] = hdsm_assign_stats{};
  }
  if (apply && n > 0) {  // (no mission is on: the goals of the path step's host copy are the current ones)
    std::vector<double> goals(d->path.goals);
    for (int k = 0; k < n; ++k)
      if (own[(size_t)k] >= 0)
        for (int c = 0; c < 3; ++c) goals[3 * (size_t)k + c] = slots[3 * (size_t)own[(size_t)k] + c];
    if (int rg = hdsm_dswarm_set_goals(dswarm, goals.data())) return rg;
  }
  if (slot_of) std::copy(own.begin(), own.end(), slot_of);
  if (stats) std::copy(st.begin(), st.end(), stats);
  return HDSM_OK;
}
