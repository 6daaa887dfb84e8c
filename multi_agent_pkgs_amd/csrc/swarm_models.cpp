// swarm_models.cpp — the models the host mirror flies beside the round (include/hdsm_swarm.h): the flight audit, neighbour groups,
// imperfect tracking, commands for the vehicle, the vehicle in the loop and missions, each with its entry points and its step of
// hdsm_swarm_commit. Pure host C++.
#include <algorithm>

#include "audit_core.h"
#include "command_core.h"
#include "hdsm_internal.h"
#include "swarm_host.h"
#include "track_core.h"
#include "vehicle_core.h"

using namespace hdsm_mirror;

// the state flown in place of traj_curr[step_plan] (track_core.h); the published record stays the plan
void hdsm_mirror::track_commit(Swarm& sw) {
  Track& t = sw.track;
  if (!t.on) return;
  const double T = (double)sw.cfg.step_plan * sw.prm.dt;
  for (int k = 0; k < sw.n_local; ++k) {
    AgentS& ag = sw.agents[k];
    if (!ag.has_traj) continue;
    double from[9], to[9];
    for (int c = 0; c < 9; ++c) from[c] = ag.traj_curr[sw.cfg.step_plan][c];
    hdsm_track::flown_state(t.model, ag.id, t.q, T, from, to);
    for (int c = 0; c < 9; ++c) ag.state_curr[c] = to[c];
    hdsm_track::book(t.rec[(size_t)k], hdsm_track::pos_dist(from, to), hdsm_track::vel_dist(from, to), false);
  }
  ++t.q;
}

// state_curr of before the commit: what the yaw step looks from (AC:177 comes before AC:233)
std::vector<double> hdsm_mirror::commands_before(const Swarm& sw) {
  std::vector<double> before;
  if (sw.cmd.on)
    for (int k = 0; k < sw.n_local; ++k) before.insert(before.end(), sw.agents[k].state_curr, sw.agents[k].state_curr + 9);
  return before;
}

// the yaw step, the setpoints of the interval about to be flown and the pose the round ends in (command_core.h)
void hdsm_mirror::commands_commit(Swarm& sw, const std::vector<double>& before, const int32_t* status) {
  Commands& m = sw.cmd;
  if (!m.on) return;
  const int step = sw.cfg.step_plan;
  for (int k = 0; k < sw.n_local; ++k) {
    const AgentS& ag = sw.agents[k];
    const int valid = !ag.has_traj ? 0 : (status[k] != HDSM_NO_SOLUTION ? 1 : 2);
    const bool has_ref = ag.n_ref > m.yaw_idx;
    double& yaw = m.yaw[(size_t)k];
    int stepped = 0;
    yaw = hdsm_cmd::agent_round(yaw, has_ref, ag.traj_ref[has_ref ? m.yaw_idx : 0], &before[(size_t)k * 9], &ag.traj_curr[0][0], ag.state_curr,
                                valid, step, m.k_p_yaw, sw.prm.dt, &m.setpoint[(size_t)k * step], &m.pose[(size_t)k], &stepped);
    m.stats[stepped ? 0 : 1] += 1;
  }
}

// the vehicles fly the setpoints commands_commit has just written (vehicle_core.h): state_curr takes the flown state, the track record
// the sample, the pose the vehicle's own attitude
void hdsm_mirror::vehicle_commit(Swarm& sw) {
  Vehicle& v = sw.veh;
  if (!v.on) return;
  const int step = sw.cfg.step_plan;
  for (int k = 0; k < sw.n_local; ++k) {
    AgentS& ag = sw.agents[k];
    double start[9], planned[9], flown[9], d, dvel;
    for (int c = 0; c < 9; ++c) start[c] = ag.traj_curr[0][c], planned[c] = ag.state_curr[c];
    int n_thrust = 0, n_rate = 0;
    const int ok = hdsm_veh::agent_round(v.m, ag.id, v.q, step, sw.prm.dt, start, &sw.cmd.setpoint[(size_t)k * step], planned, v.state[(size_t)k], flown,
                                         &d, &dvel, &sw.cmd.pose[(size_t)k], &n_thrust, &n_rate);
    for (int c = 0; c < 9; ++c) ag.state_curr[c] = flown[c];
    if (ok) hdsm_track::book(sw.track.rec[(size_t)k], d, dvel, false);
    v.stats[0] += ok, v.stats[1] += 1 - ok, v.stats[2] += n_thrust, v.stats[3] += n_rate;
  }
  ++v.q;
}

// the mission judges state_curr as the commit, the tracking model and the vehicle left it (mission_core.h); an agent that turns to
// another waypoint gets it as its goal and plans a path at the start of the next round
void hdsm_mirror::mission_commit(Swarm& sw) {
  Mission& ms = sw.mission;
  if (!ms.on) return;
  ms.last = hdsm_mission_rule::tally_identity();
  for (int k = 0; k < sw.n_local; ++k) {
    AgentS& ag = sw.agents[k];
    double goal[3];
    int turn = 0;
    const int arrived = hdsm_mission_rule::step(ms.m, ms.rec[(size_t)k], ag.state_curr, &ms.waypoints[(size_t)k * 3 * ms.m.n_wp], ms.count[(size_t)k], ms.q,
                                                goal, &turn);
    if (turn) ag.goal = V3{{goal[0], goal[1], goal[2]}}, sw.path.due[(size_t)k] = 1;
    hdsm_mission_rule::tally_add(ms.last, ms.rec[(size_t)k], arrived);
  }
  ++ms.q;
}

extern "C" {

// Missions on the host mirror (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_swarm_set_mission(void* swarm, const hdsm_mission* m, const double* waypoints, const int32_t* count) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  Mission& ms = sw->mission;
  if (!m) {
    ms.on = false;
    return HDSM_OK;
  }
  if (!hdsm_mission_rule::setting_valid(m, sw->n_local, waypoints, count)) return HDSM_ERR_BAD_ARG;
  const size_t n = (size_t)sw->n_local;
  ms.m = *m, ms.q = 0, ms.last = hdsm_mission_rule::tally_identity();
  ms.waypoints.assign(waypoints, waypoints + n * 3 * (size_t)m->n_wp), ms.count.assign(count, count + n);
  ms.rec.assign(n, hdsm_mission_record{});
  for (size_t k = 0; k < n; ++k) {
    AgentS& ag = sw->agents[k];
    const double* w0 = &ms.waypoints[k * 3 * (size_t)m->n_wp];
    hdsm_mission_rule::reset(ms.rec[k]);
    ag.goal = V3{{w0[0], w0[1], w0[2]}}, sw->path.due[k] = 1;
  }
  ms.on = ms.ever = true;
  return HDSM_OK;
}

int hdsm_swarm_mission_records(void* swarm, hdsm_mission_record* out) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->mission.ever || (!out && sw->n_local)) return HDSM_ERR_BAD_ARG;
  std::copy(sw->mission.rec.begin(), sw->mission.rec.end(), out);
  return HDSM_OK;
}

int hdsm_swarm_mission_summary(void* swarm, hdsm_mission_summary* out) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->mission.ever || !out) return HDSM_ERR_BAD_ARG;
  *out = hdsm_mission_rule::summary_of(sw->mission.last, sw->mission.q - 1, sw->n_local);
  return HDSM_OK;
}

int hdsm_swarm_mission_due(void* swarm, uint8_t* due, double* goals) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  if (due) std::copy(sw->path.due.begin(), sw->path.due.end(), due);
  if (goals)
    for (int k = 0; k < sw->n_local; ++k)
      for (int c = 0; c < 3; ++c) goals[3 * (size_t)k + c] = sw->agents[k].goal[c];
  return HDSM_OK;
}

// A vehicle in the loop on the host mirror (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_swarm_set_vehicle(void* swarm, const hdsm_vehicle* m) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  Vehicle& v = sw->veh;
  if (!m) {
    v.on = false;
    return HDSM_OK;
  }
  if (!hdsm_veh::settings_valid(m) || !sw->cmd.on || sw->track.on) return HDSM_ERR_BAD_ARG;
  sw->track.ready(sw->n_local);
  if (!v.on) {  // a switch-on (the vehicle was off, or never there, while the agents moved): every vehicle seated on its agent's state and yaw
    v.state.assign((size_t)sw->n_local, hdsm_vehicle_state{});
    for (int k = 0; k < sw->n_local; ++k) hdsm_veh::seat(*m, sw->agents[k].state_curr, sw->cmd.yaw[(size_t)k], v.state[(size_t)k]);
    v.ever = true;
  }
  v.m = *m, v.q = 0, v.on = true;
  return HDSM_OK;
}

int hdsm_swarm_vehicle_states(void* swarm, hdsm_vehicle_state* out) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->veh.ever || (!out && sw->n_local)) return HDSM_ERR_BAD_ARG;
  std::copy(sw->veh.state.begin(), sw->veh.state.end(), out);
  return HDSM_OK;
}

// Imperfect tracking on the host mirror (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_swarm_set_tracking(void* swarm, const hdsm_tracking* m) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || (m && !hdsm_track::model_valid(m))) return HDSM_ERR_BAD_ARG;
  if (m && sw->veh.on) return HDSM_ERR_BAD_ARG;  // (a vehicle is what deviates from the plan)
  sw->track.on = m != nullptr;
  if (m) sw->track.model = *m, sw->track.q = 0, sw->track.ready(sw->n_local);
  return HDSM_OK;
}

int hdsm_swarm_set_states(void* swarm, const double* states, const uint8_t* mask) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || (!states && sw->n_local)) return HDSM_ERR_BAD_ARG;
  sw->track.ready(sw->n_local);
  for (int k = 0; k < sw->n_local; ++k) {
    const double* to = states + (size_t)k * 9;
    if ((mask && !mask[k]) || !hdsm_track::finite9(to)) continue;
    AgentS& ag = sw->agents[k];
    double from[9];
    for (int c = 0; c < 9; ++c) from[c] = ag.state_curr[c], ag.state_curr[c] = to[c];
    hdsm_track::book(sw->track.rec[(size_t)k], hdsm_track::pos_dist(from, to), hdsm_track::vel_dist(from, to), true);
    if (sw->veh.ever) hdsm_veh::seat(sw->veh.m, to, sw->cmd.yaw[(size_t)k], sw->veh.state[(size_t)k]);  // the vehicle is where it was measured
  }
  return HDSM_OK;
}

int hdsm_swarm_track_records(void* swarm, hdsm_track_record* out) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || (!out && sw->n_local)) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k) out[k] = (size_t)k < sw->track.rec.size() ? sw->track.rec[(size_t)k] : hdsm_track_record{};
  return HDSM_OK;
}

// Commands for the vehicle on the host mirror (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_swarm_set_commands(void* swarm, int32_t on, int32_t yaw_idx, double k_p_yaw, const double* yaw0) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  if (on && !hdsm_cmd::settings_valid(yaw_idx, sw->prm.n_hor, k_p_yaw, yaw0, sw->n_local)) return HDSM_ERR_BAD_ARG;
  if (!on && sw->veh.on) return HDSM_ERR_BAD_ARG;  // (the vehicle needs the setpoints and the yaw)
  Commands& m = sw->cmd;
  const size_t n = (size_t)sw->n_local;
  m.ready(n, sw->cfg.step_plan);
  m.on = on != 0;
  if (on) {
    m.yaw_idx = yaw_idx, m.k_p_yaw = k_p_yaw;
    for (size_t k = 0; k < n; ++k) m.yaw[k] = yaw0 ? yaw0[k] : 0.0;
  }
  return HDSM_OK;
}

int hdsm_swarm_commands(void* swarm, hdsm_command* setpoint, hdsm_command* pose, double* yaw) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->cmd.ever) return HDSM_ERR_BAD_ARG;
  const Commands& m = sw->cmd;
  if (setpoint) std::copy(m.setpoint.begin(), m.setpoint.end(), setpoint);
  if (pose) std::copy(m.pose.begin(), m.pose.end(), pose);
  if (yaw) std::copy(m.yaw.begin(), m.yaw.end(), yaw);
  return HDSM_OK;
}

// ---- the flight audit of the host mirror (audit_core.h) ----
int hdsm_swarm_set_audit(void* swarm, int32_t on, double sep_warn) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !(sep_warn > 0)) return HDSM_ERR_BAD_ARG;
  Audit& a = sw->audit;
  if (on && !a.ever) {
    a.flight.resize((size_t)sw->n_local);
    for (hdsm_flight_report& r : a.flight) hdsm_audit::empty_report(&r);
    a.ever = true;
  }
  a.on = on != 0, a.sep_warn = sep_warn;
  return HDSM_OK;
}

int hdsm_swarm_get_audit(void* swarm, int32_t* on, double* sep_warn) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !on) return HDSM_ERR_BAD_ARG;
  *on = sw->audit.on ? 1 : 0;
  if (sep_warn) *sep_warn = sw->audit.sep_warn;
  return HDSM_OK;
}

int hdsm_swarm_audit(void* swarm, const double* plans_all, const uint8_t* has_plan) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !plans_all || !has_plan || !sw->audit.on) return HDSM_ERR_BAD_ARG;
  Audit& a = sw->audit;
  a.last.resize((size_t)sw->n_local);
  const int rc = hdsm_internal_audit_host_grouped(sw->n_rob, plans_all, has_plan, sw->prm.n_hor, sw->cfg.step_plan, sw->first_id, sw->n_local,
                                                  sw->prm.drone_radius, sw->prm.drone_z_offset, sw->world.data(), sw->world.dim,
                                                  sw->world.origin, sw->cfg.voxel_size, sw->groups.range.empty() ? nullptr : sw->groups.range.data(),
                                                  a.last.data());
  if (rc) return rc;
  const double warn2 = a.sep_warn * a.sep_warn;
  for (int k = 0; k < sw->n_local; ++k)
    if (has_plan[sw->first_id + k]) hdsm_audit::accumulate(&a.flight[k], a.last[k], sw->cfg.step_plan, warn2);
  return HDSM_OK;
}

int hdsm_swarm_flight_report(void* swarm, hdsm_flight_report* report) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->audit.ever || (sw->n_local && !report)) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k) report[k] = sw->audit.flight[k];
  return HDSM_OK;
}

// ---- neighbour groups of the host mirror (ABI 1.8; the definition: include/hdsm.h, hdsm_set_groups) ----
int hdsm_swarm_set_groups(void* swarm, int32_t n_groups, const int32_t* group_start) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || n_groups < 0) return HDSM_ERR_BAD_ARG;
  Groups& g = sw->groups;
  if (n_groups == 0 || !group_start) {
    g.start.clear(), g.range.clear();
    return HDSM_OK;
  }
  if (group_start[0] != 0 || group_start[n_groups] != sw->n_rob) return HDSM_ERR_BAD_ARG;
  for (int i = 0; i < n_groups; ++i)
    if (group_start[i + 1] <= group_start[i]) return HDSM_ERR_BAD_ARG;
  g.start.assign(group_start, group_start + n_groups + 1);
  g.range.assign((size_t)sw->n_rob * 2, 0);
  for (int i = 0; i < n_groups; ++i)
    for (int k = group_start[i]; k < group_start[i + 1]; ++k) g.range[2 * (size_t)k] = group_start[i], g.range[2 * (size_t)k + 1] = group_start[i + 1];
  return HDSM_OK;
}

}  // extern "C"
