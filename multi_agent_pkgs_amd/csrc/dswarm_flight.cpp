// dswarm_flight.cpp — the flight in and out of the device-resident loop: the host mirror's state onto the device at hdsm_dswarm_create
// (take_over) and back (hdsm_dswarm_download, hand_back), the plans buffer up and down, and the goals a caller sets between rounds.
// Copies and bookkeeping only: nothing here launches a kernel.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "dswarm.h"
#include "hdsm_internal.h"
#include "swarm_host.h"

using namespace hdsm_dswarm;

int hdsm_dswarm::upload_goals_and_due(DSwarm* d) {
  PathStep& p = d->path;
  std::vector<int32_t> idx;
  for (int k = 0; k < d->n_local; ++k)
    if (p.due[(size_t)k]) idx.push_back(k);
  p.n_due = (int)idx.size();
  HIP_TRY(hipMemcpy(p.d_goals.get(), p.goals.data(), p.goals.size() * sizeof(double), hipMemcpyHostToDevice));
  if (p.n_due) HIP_TRY(hipMemcpy(p.d_due.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return HDSM_OK;
}

// The mirror's flight becomes the device's (hdsm_dswarm_create, after alloc_round_buffers): the path step's phase and pending agents,
// the clearance mode, the agent states, ids and goals, the world (hworld: the mirror's grid or NULL), the partition, the audit's
// setting and record, the command setting and yaw, the vehicle setting, round and states. Each is read from the mirror's member struct (swarm_host.h).
int hdsm_dswarm::take_over(DSwarm& d, void* swarm, const int8_t* hworld) {
  const hdsm_mirror::Swarm& sw = *hdsm_mirror::as_swarm(swarm);
  const size_t n = (size_t)d.n_local;
  PathStep& p = d.path;
  p.period = sw.path.period, p.round = sw.path.round, p.due = sw.path.due;
  p.goals.assign(n * 3, 0.0);
  if (const hdsm_path::DmpMask* mask = sw.path.dmp()) {
    p.dmp = true, p.dmp_rn = mask->rn;
    HIP_TRY(p.d_dmp_rows.alloc_zeroed(sizeof mask->rows / sizeof mask->rows[0]));
    HIP_TRY(hipMemcpy(p.d_dmp_rows.get(), mask->rows, sizeof mask->rows, hipMemcpyHostToDevice));
  }
  if (n) {
    HIP_TRY(hipMemcpy(d.d_agents.get(), sw.agents.data(), n * sizeof(AgentS), hipMemcpyHostToDevice));
    // the agent ids of the shard (a contiguous block), the goals, and the agents the mirror had marked due (hdsm_swarm_set_goals before the dswarm)
    std::vector<int32_t> ids(n, 0);
    for (size_t k = 0; k < n; ++k) {
      for (int q = 0; q < 3; ++q) p.goals[3 * k + q] = sw.agents[k].goal[q];
      ids[k] = d.first + (int)k;
    }
    HIP_TRY(hipMemcpy(d.d_id.get(), ids.data(), n * 4, hipMemcpyHostToDevice));
    if (int rc = upload_goals_and_due(&d)) return rc;
  }
  if (hworld) HIP_TRY(hipMemcpy(d.d_world.get(), hworld, d.voxels(), hipMemcpyHostToDevice));
  d.c.world = d.d_world.get();
  {  // the mirror's partition goes onto the solver handle (none: the handle's is cleared) and, for the audit, into a range table
    const int ng = sw.groups.n();
    d.grouped = ng > 0;
    d.group_start = d.grouped ? sw.groups.start : std::vector<int32_t>{0, d.n_rob};
    if (int rc = hdsm_set_groups(d.solver, ng, d.grouped ? d.group_start.data() : nullptr))
      return fail(rc, std::string("hdsm_set_groups: ") + hdsm_last_error());
    HIP_TRY(hipSetDevice(d.device));  // (the handle may live on another device)
    if (d.grouped) {
      const size_t G = (size_t)d.slots();
      std::vector<int32_t> table(2 * G + 2, 0);
      for (int g = 0; g < ng; ++g)
        for (int k = d.group_start[g]; k < d.group_start[g + 1]; ++k) table[2 * (size_t)k] = d.group_start[g], table[2 * (size_t)k + 1] = d.group_start[g + 1];
      HIP_TRY(d.d_range.alloc(table.size()));
      HIP_TRY(hipMemcpy(d.d_range.get(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
  }
  d.audit.sep_warn = sw.audit.sep_warn;  // the audit's setting and record of the mirror (a flight taken over keeps its record)
  if (sw.audit.ever) {
    d.audit.on = sw.audit.on;
    if (int rc = audit_setup(&d, sw.audit.flight.data())) return rc;
  }
  if (sw.cmd.on)  // the command setting and yaw of the mirror (a flight taken over keeps its yaw)
    if (int rc = commands_setup(&d, true, sw.cmd.yaw_idx, sw.cmd.k_p_yaw, sw.cmd.yaw.data())) return rc;
  if (sw.veh.on)  // the vehicle setting, round and states of the mirror (a vehicle has memory: a flight taken over does not jump)
    if (int rc = vehicle_setup(&d, sw.veh.m, sw.veh.q, sw.veh.state.data())) return rc;
  if (sw.mission.on)  // the mission setting, table, records and round of the mirror; the agents it had due become the device's flags
    if (int rc = mission_setup(&d, sw.mission.m, sw.mission.waypoints.data(), sw.mission.count.data(), sw.mission.q, sw.mission.rec.data(), p.due.data()))
      return rc;
  return HDSM_OK;
}

// The device's flight back into the mirror (hdsm_dswarm_download; the device is idle): the agent states, the path step's phase,
// pending agents and goals, the audit's setting and record, the command setting and yaw, the vehicle setting, round and states. Each piece goes through the adopt of the
// mirror's member struct, which keeps that struct's invariants.
int hdsm_dswarm::hand_back(DSwarm& d, void* swarm) {
  hdsm_mirror::Swarm& sw = *hdsm_mirror::as_swarm(swarm);
  const size_t n = (size_t)d.n_local;
  std::unique_ptr<AgentS[]> tmp(new (std::nothrow) AgentS[n]);
  if (!tmp) return fail(HDSM_ERR_DEVICE, "out of host memory");
  int rc = hipMemcpy(tmp.get(), d.d_agents.get(), n * sizeof(AgentS), hipMemcpyDeviceToHost) == hipSuccess
               ? hdsm_swarm_import_state(swarm, tmp.get(), d.n_local)
               : HDSM_ERR_DEVICE;
  std::vector<uint8_t> due = d.path.due;
  if (rc == HDSM_OK && d.mission.on) {  // the device's flags are the agents due; the goals live on the device; the mission goes back whole
    Mission& ms = d.mission;
    const size_t W = n * 3 * (size_t)ms.m.n_wp;
    std::vector<double> wps(W);
    std::vector<int32_t> count(n);
    std::vector<hdsm_mission_record> rec(n);
    if (mission_pull_goals(&d) != HDSM_OK || hipMemcpy(due.data(), ms.d_flag.get(), n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(wps.data(), ms.d_wps.get(), W * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(count.data(), ms.d_count.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rec.data(), ms.d_rec.get(), n * sizeof(hdsm_mission_record), hipMemcpyDeviceToHost) != hipSuccess)
      rc = HDSM_ERR_DEVICE;
    else sw.mission.adopt(ms.m, ms.q, std::move(wps), std::move(count), std::move(rec));
  } else if (rc == HDSM_OK && sw.mission.on && d.mission.ready()) {
    sw.mission.on = false;  // (switched off on the device)
  }
  for (size_t k = 0; k < n; ++k) due[k] |= d.path.due[k];  // (merged with the host's list, which is empty while a mission is on)
  if (rc == HDSM_OK) rc = sw.path.adopt(d.path.period, d.path.round, due);
  if (rc == HDSM_OK) sw.adopt_goals(d.path.goals);
  if (rc == HDSM_OK && d.audit.ever) {
    std::vector<hdsm_flight_report> rep(n);
    if (hipMemcpy(rep.data(), d.audit.d_report.get(), n * sizeof(hdsm_flight_report), hipMemcpyDeviceToHost) != hipSuccess) rc = HDSM_ERR_DEVICE;
    else rc = sw.audit.adopt(d.audit.on, d.audit.sep_warn, std::move(rep));
  }
  if (rc == HDSM_OK && d.cmd.ready()) {
    std::vector<double> yaw(n);
    if (hipMemcpy(yaw.data(), d.cmd.d_yaw.get(), n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = HDSM_ERR_DEVICE;
    else sw.cmd.adopt(d.cfg.step_plan, d.cmd.on, d.cmd.yaw_idx, d.cmd.k_p_yaw, yaw);
  }
  if (rc == HDSM_OK && d.veh.ready()) {
    std::vector<hdsm_vehicle_state> vs(n);
    if (hipMemcpy(vs.data(), d.veh.d_state.get(), n * sizeof(hdsm_vehicle_state), hipMemcpyDeviceToHost) != hipSuccess) rc = HDSM_ERR_DEVICE;
    else sw.veh.adopt(d.veh.on, d.veh.m, d.veh.q, std::move(vs)), sw.track.ready(d.n_local);
  }
  return rc ? fail(rc, "state download failed") : HDSM_OK;
}

extern "C" {

// GoalCallback (AC:2380-2388) for the shard: goals [n_local][3]; the agents whose goal changed plan a new path at the start of
// the next round (k_path). Synchronises the device.
int hdsm_dswarm_set_goals(void* dswarm, const double* goals) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!goals && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (d->mission.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_goals: a mission is on (hdsm_dswarm_set_mission): the goals are its waypoints");
  if (d->n_local == 0) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  PathStep& p = d->path;
  for (int k = 0; k < d->n_local; ++k) {
    double* g = &p.goals[3 * (size_t)k];
    const double* ng = goals + 3 * (size_t)k;
    if (g[0] == ng[0] && g[1] == ng[1] && g[2] == ng[2]) continue;
    g[0] = ng[0], g[1] = ng[1], g[2] = ng[2];
    p.due[k] = 1;
  }
  return upload_goals_and_due(d);
}

// out[0] agents planned by k_path since hdsm_dswarm_create, out[1] of them without a new path, out[2] launches of k_path.
// Synchronises the device.
int hdsm_dswarm_path_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (int rc = device_idle(d)) return rc;
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, d->path.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost));
  out[0] = (int64_t)cnt[0], out[1] = (int64_t)cnt[1], out[2] = d->path.launches;
  if (d->mission.ready()) {  // (the device-sized launches of a mission that planned somebody are counted where that is known: on the device)
    unsigned long long planned[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(planned, d->mission.d_planned.get(), sizeof planned, hipMemcpyDeviceToHost));
    out[2] += (int64_t)planned[2];
  }
  return HDSM_OK;
}

int hdsm_dswarm_plans_device(void* dswarm, void** d_plans, void** d_has) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !d_plans || !d_has) return fail(HDSM_ERR_BAD_ARG, "null argument");
  *d_plans = d->d_plans.get(), *d_has = d->d_has.get();
  return HDSM_OK;
}

int hdsm_dswarm_download_raw(void* dswarm, double* plans_all_raw, double* send_raw) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (int rc = device_idle(d)) return rc;
  const size_t L = (size_t)d->per, G = (size_t)d->slots(), rec = (size_t)d->rec();
  if (plans_all_raw && G) HIP_TRY(hipMemcpy(plans_all_raw, d->d_plans.get(), G * rec * 8, hipMemcpyDeviceToHost));
  if (send_raw && L) HIP_TRY(hipMemcpy(send_raw, d->d_local.get(), L * rec * 8, hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_upload_plans(void* dswarm, const double* plans_all, const uint8_t* has_plan) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !plans_all || !has_plan) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (int rc = device_idle(d)) return rc;
  const size_t G = (size_t)d->slots(), rec = (size_t)d->rec(), have = (size_t)d->n_rob < G ? (size_t)d->n_rob : G;
  HIP_TRY(hipMemset(d->d_has.get(), 0, G));
  HIP_TRY(hipMemcpy(d->d_plans.get(), plans_all, have * rec * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d->d_has.get(), has_plan, have, hipMemcpyHostToDevice));
  return HDSM_OK;
}

int hdsm_dswarm_download(void* dswarm, void* swarm, double* plans_all, uint8_t* has_plan, int32_t* status, int32_t* failed_total) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (int rc = device_idle(d)) return rc;
  const size_t n = (size_t)d->n_local, G = (size_t)d->slots(), rec = (size_t)d->rec();
  if (swarm && n)
    if (int rc = hand_back(*d, swarm)) return rc;
  if (plans_all) {
    HIP_TRY(hipMemcpy(plans_all, d->d_plans.get(), G * rec * 8, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < G; ++k)
      if (plans_all[k * rec] != plans_all[k * rec]) plans_all[k * rec] = 0.0;  // the sentinel is for the wire only
  }
  if (has_plan) HIP_TRY(hipMemcpy(has_plan, d->d_has.get(), G, hipMemcpyDeviceToHost));
  if (status && n) HIP_TRY(hipMemcpy(status, d->d_status.get(), n * 4, hipMemcpyDeviceToHost));
  if (failed_total) HIP_TRY(hipMemcpy(failed_total, d->d_fails.get(), 4, hipMemcpyDeviceToHost));
  return HDSM_OK;
}

}  // extern "C"
