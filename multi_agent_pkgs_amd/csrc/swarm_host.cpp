// swarm_host.cpp — host-side planner state around the solve (see include/hdsm_swarm.h): the round (create, prepare, commit) and the
// reference restatement. The mirror's state is in swarm_host.h; what runs between rounds is in swarm_world.cpp, swarm_models.cpp,
// swarm_router.cpp and swarm_flight.cpp.
// AC = multi_agent_planner/src/agent_class.cpp of lis-epfl/multi_agent_pkgs. Pure host C++.
#include <cmath>
#include <ctime>
#include <new>
#include <vector>

#include "swarm_host.h"

using namespace hdsm_mirror;

namespace {

inline double cpu_ms_since(clock_t t0) { return (double)(clock() - t0) / CLOCKS_PER_SEC * 1e3; }

// GetVelocityLimit, AC:1805-1817
double velocity_limit(const hdsm_swarm_config& c, double occ, double dist) {
  if (occ < 0) occ = 0;
  if (occ > 100) occ = 100;
  const double alpha = 1 - std::pow(occ / 100, c.sens_pot) * (1 / std::exp(c.sens_dist * dist));
  return c.path_vel_min + (c.path_vel_max - c.path_vel_min) * alpha;
}

// ComputePathVelocity, AC:1695-1803: empty world -> only the neighbour term (AC:1769-1801) is active
hdsm_ref_config ref_config(const Swarm& sw) {
  return {sw.cfg.path_vel_min, sw.cfg.path_vel_max, sw.cfg.sens_dist, sw.cfg.sens_pot, sw.cfg.sens_other_agents, sw.cfg.path_vel_dec};
}

double compute_path_velocity(const Swarm& sw, const hdsm_sw::Cfg& cc, const AgentS& ag, const std::vector<V3>& path, const double* plans_all,
                             const uint8_t* has_plan) {
  const int N = sw.prm.n_hor;
  // voxel / potential-field term (AC:1709-1766) on the agent's local grid, then the neighbour term (AC:1769-1801)
  double path_vel = hdsm_sw::voxel_velocity_cap(cc, ref_config(sw), hdsm_sw::local_grid_origin(cc, ag), path.data(), (int)path.size());
  int g_lo, g_hi;  // the agent's neighbours: its group (everybody without a partition)
  sw.neighbour_range(ag.id, &g_lo, &g_hi);
  for (int i = 0; i < (ag.has_traj ? N + 1 : 0); ++i) {
    const V3 start = {{ag.traj_curr[i][0], ag.traj_curr[i][1], ag.traj_curr[i][2]}};
    const double occ = 100 * std::pow(sw.cfg.sens_other_agents, (double)i);
    for (int j = g_lo; j < g_hi; ++j) {
      if (j == ag.id || !has_plan[j]) continue;
      const double* st = plans_all + ((size_t)j * (N + 1) + i) * 9;
      const double d = norm(sub(start, V3{{st[0], st[1], st[2]}}));
      const double v = velocity_limit(sw.cfg, occ, d);
      if (v < path_vel) path_vel = v;
    }
  }
  return path_vel;
}

// SamplePath, AC:1591-1663
std::vector<V3> sample_path(const Swarm& sw, const hdsm_sw::Cfg& cc, AgentS& ag, const std::vector<V3>& path, const double* plans_all,
                            const uint8_t* has_plan) {
  const int N = sw.prm.n_hor;
  std::vector<V3> ref;
  if (path.size() < 2) {
    for (int i = 0; i < N; ++i) ref.push_back(path[0]);
    return ref;
  }
  ag.path_vel = compute_path_velocity(sw, cc, ag, path, plans_all, has_plan);
  const double samp_dist = ag.path_vel * sw.prm.dt;
  size_t path_idx = 1;
  int ref_idx = 0;
  V3 curr = path[0];
  ref.push_back(path.front());
  double limit = samp_dist;
  while (ref_idx < N) {
    const V3 diff = sub(path[path_idx], curr);
    const double dist_next = norm(diff);
    if (dist_next > limit) {
      curr = hdsm_sw::step_along(curr, limit, diff, dist_next);
      ref.push_back(curr);
      ++ref_idx;
      limit = std::fmax(0.0, samp_dist - sw.cfg.path_vel_dec * sw.prm.dt);
    } else {
      curr = path[path_idx];
      if (++path_idx == path.size()) {
        for (int i = ref_idx; i < N; ++i) ref.push_back(path.back());
        return ref;
      }
      limit -= dist_next;
    }
  }
  return ref;
}

std::vector<V3> reference_polyline(const AgentS& ag) {
  V3 buf[hdsm_sw::PATH_PTS + 1];
  const int n = hdsm_sw::reference_polyline(ag, buf);
  return std::vector<V3>(buf, buf + n);
}

// GenerateReferenceTrajectory, AC:1449-1553
void generate_reference(const Swarm& sw, const hdsm_sw::Cfg& cc, AgentS& ag, const double* plans_all, const uint8_t* has_plan) {
  const std::vector<V3> path_samp = reference_polyline(ag);  // AC:1459-1496
  std::vector<V3> pts = sample_path(sw, cc, ag, path_samp, plans_all, has_plan);
  // velocity reference, AC:1527-1547 (points backwards along the path; reproduced as is)
  ag.n_ref = (int)pts.size();
  double v[3] = {0, 0, 0};
  for (size_t i = 0; i < pts.size(); ++i) {
    if (i + 1 < pts.size()) {
      const V3 d = sub(pts[i], pts[i + 1]);
      const double dist = norm(d);
      for (int k = 0; k < 3; ++k) v[k] = dist > 1e-2 ? ag.path_vel * d[k] / dist : 0.0;
    }
    for (int k = 0; k < 3; ++k) ag.traj_ref[i][k] = pts[i][k], ag.traj_ref[i][3 + k] = v[k];
  }
  hdsm_sw::keep_only_free(cc, hdsm_sw::local_grid_origin(cc, ag), ag.path_vel, ag.traj_ref, ag.n_ref);  // AC:1512-1514
}

// GenerateSafeCorridor (AC:165) of every agent, with its CPU time (comp_time_sc_, AC:1446)
void corridor_round(Swarm& sw, const hdsm_sw::Cfg& cc) {
  for (int k = 0; k < sw.n_local; ++k) {
    const clock_t t0 = clock();
    hdsm_sw::corridor_step(cc, sw.agents[k], sw.work.get(), sw.bits.data());
    sw.extra[k].sc_ms = cpu_ms_since(t0);
  }
}

// f3: the records Agent::TrajPlanningIteration keeps (AC:193-245). The separating planes are generated inside the fused
// launch: its duration (hdsm_swarm_record_solve_ms) is booked as comp_time_opt_, comp_time_tasc_ is 0.
void book_round(Swarm& sw) {
  Round& r = sw.round;
  const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r.t0).count();
  const double stamp = (double)(r.idx + 1) * sw.prm.dt * sw.cfg.step_plan;
  for (int k = 0; k < sw.n_local; ++k) {
    const AgentX& x = sw.extra[k];
    hdsm_stats_add(x.stats, HDSM_STAT_SC, x.sc_ms);
    hdsm_stats_add(x.stats, HDSM_STAT_TASC, 0.0);
    hdsm_stats_add(x.stats, HDSM_STAT_OPT, r.solve_ms);
    hdsm_stats_add(x.stats, HDSM_STAT_TOT, x.sc_ms + x.ref_ms + r.solve_ms);
    hdsm_stats_add(x.stats, HDSM_STAT_TOT_WALL, wall_ms);
    hdsm_stats_add_state(x.stats, stamp, sw.agents[k].state_curr, 9);
  }
  ++r.idx;
}

}  // namespace

extern "C" {

void hdsm_swarm_default_config(hdsm_swarm_config* c) {
  if (!c) return;
  c->path_vel_min = 4.5, c->path_vel_max = 9.0, c->sens_dist = 0.05, c->sens_pot = 0.18;
  c->sens_other_agents = 1.0, c->path_vel_dec = 0.0, c->thresh_dist = 1.0, c->voxel_size = 0.3;
  c->grid_range[0] = 20.0, c->grid_range[1] = 20.0, c->grid_range[2] = 6.0, c->grid_z_min = 0.0;
  c->n_it_decomp = 42, c->step_plan = 1, c->use_cvx_new = 0, c->reserved0 = 0;
}

int hdsm_swarm_create(const hdsm_params* prm, const hdsm_swarm_config* cfg, int32_t n_rob, int32_t first_id,
                      int32_t n_local, const double* starts, const double* goals, void** swarm) {
  if (!prm || !cfg || !starts || !goals || !swarm) return HDSM_ERR_BAD_ARG;
  if (n_rob < 1 || n_local < 0 || first_id < 0 || first_id + n_local > n_rob) return HDSM_ERR_BAD_ARG;
  if (prm->n_hor < 2 || prm->n_hor > HDSM_MAX_HOR || prm->poly_hor < 1 || prm->poly_hor > HDSM_MAX_POLY)
    return HDSM_ERR_BAD_ARG;
  if (prm->max_rows_static < 6 || cfg->step_plan < 1 || cfg->step_plan > prm->n_hor) return HDSM_ERR_BAD_ARG;
  Swarm* sw = new (std::nothrow) Swarm;
  if (!sw) return HDSM_ERR_DEVICE;
  sw->prm = *prm, sw->cfg = *cfg, sw->n_rob = n_rob, sw->first_id = first_id, sw->n_local = n_local;
  sw->agents.assign(n_local, AgentS{});
  sw->extra.assign(n_local, AgentX{});
  sw->path.due.assign(n_local, 0);
  for (int k = 0; k < n_local; ++k) {
    AgentS& a = sw->agents[k];
    a.id = first_id + k;
    for (int ax = 0; ax < 3; ++ax) a.start[ax] = starts[3 * k + ax], a.goal[ax] = goals[3 * k + ax];
    a.n_path = 2, a.path[0] = a.start, a.path[1] = a.goal;
    sw->extra[k].stats = hdsm_stats_create(a.id, n_rob);
    for (int ax = 0; ax < 3; ++ax) a.state_curr[ax] = a.start[ax];
  }
  *swarm = sw;
  return HDSM_OK;
}

void hdsm_swarm_destroy(void* swarm) { delete as_swarm(swarm); }

int hdsm_swarm_prepare(void* swarm, const double* plans_all, const uint8_t* has_plan, int32_t* agent_id,
                       double* state_curr, double* traj_ref, int32_t* n_poly, int32_t* n_rows_static,
                       double* A_static, double* b_static) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !plans_all || !has_plan || !agent_id || !state_curr || !traj_ref || !n_poly || !n_rows_static ||
      !A_static || !b_static)
    return HDSM_ERR_BAD_ARG;
  const int N = sw->prm.n_hor, P = sw->prm.poly_hor, RS = sw->prm.max_rows_static;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  sw->round.t0 = std::chrono::steady_clock::now();
  sw->round.solve_ms = 0;
  if (!sw->round.corridor_done) {
    path_round(*sw, cc);  // (UpdatePath's thread, AC:261-454, once per round before the corridor)
    corridor_round(*sw, cc);
  }
  sw->round.corridor_done = false;
  for (int k = 0; k < sw->n_local; ++k) {
    AgentS& ag = sw->agents[k];
    const clock_t t0 = clock();
    if (!ag.external_ref) generate_reference(*sw, cc, ag, plans_all, has_plan);  // AC:171 (or done on the device, f1)
    sw->extra[k].ref_ms = cpu_ms_since(t0);
    ag.external_ref = 0;
    hdsm_sw::fill_inputs(cc, ag, agent_id + k, state_curr + 9 * (size_t)k, traj_ref + (size_t)k * N * 6, n_poly + k,
                         n_rows_static + (size_t)k * P, A_static + (size_t)k * P * RS * 3, b_static + (size_t)k * P * RS);
  }
  return HDSM_OK;
}

// GenerateSafeCorridor alone (AC:165), for callers that generate the reference elsewhere (row f1 on the device) and want the
// reference's own order: corridor from the PREVIOUS reference, then the new reference. The following hdsm_swarm_prepare of the
// same round does not repeat it.
int hdsm_swarm_prepare_corridor(void* swarm) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  path_round(*sw, cc);
  corridor_round(*sw, cc);
  sw->round.corridor_done = true;
  return HDSM_OK;
}

int hdsm_swarm_commit(void* swarm, const double* traj_out, const double* ctrl_out, const uint8_t* poly_used,
                      const int32_t* status, double* plans_local, uint8_t* has_plan_local) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !traj_out || !ctrl_out || !poly_used || !status || !plans_local || !has_plan_local)
    return HDSM_ERR_BAD_ARG;
  const int N = sw->prm.n_hor, P = sw->prm.poly_hor;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  const std::vector<double> before = commands_before(*sw);
  for (int k = 0; k < sw->n_local; ++k) {
    AgentS& ag = sw->agents[k];
    const int have_plan = hdsm_sw::commit_one(cc, ag, traj_out + (size_t)k * (N + 1) * 9, ctrl_out + (size_t)k * N * 3,
                                              poly_used + (size_t)k * P, status[k]);
    has_plan_local[k] = have_plan ? 1 : 0;
    for (int i = 0; i <= N; ++i)
      for (int c = 0; c < 9; ++c)
        plans_local[((size_t)k * (N + 1) + i) * 9 + c] = have_plan ? ag.traj_curr[i][c] : 0.0;
  }
  track_commit(*sw);
  commands_commit(*sw, before, status);
  vehicle_commit(*sw);
  mission_commit(*sw);
  book_round(*sw);
  return HDSM_OK;
}

int hdsm_swarm_record_solve_ms(void* swarm, double milliseconds) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !(milliseconds >= 0)) return HDSM_ERR_BAD_ARG;
  sw->round.solve_ms = milliseconds;
  return HDSM_OK;
}

int hdsm_swarm_shutdown(void* swarm, int32_t local_index, const char* dir, int32_t save_stats, char* report, int32_t report_cap) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || local_index < 0 || local_index >= sw->n_local) return HDSM_ERR_BAD_ARG;
  return hdsm_stats_shutdown(sw->extra[local_index].stats, dir, save_stats, report, report_cap);
}

int hdsm_swarm_reference_inputs_n(void* swarm, int32_t pmax, double* path, int32_t* n_path) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !path || !n_path || pmax < 2) return HDSM_ERR_BAD_ARG;
  const double need = sw->prm.n_hor * sw->cfg.path_vel_max * sw->prm.dt;  // SamplePath never walks further than this
  for (int k = 0; k < sw->n_local; ++k) {
    const std::vector<V3> pl = reference_polyline(sw->agents[k]);
    int n = (int)pl.size();
    if (n > pmax) {
      double len = 0;
      for (int i = 0; i + 1 < pmax; ++i) len += norm(sub(pl[i + 1], pl[i]));
      if (len <= need) return HDSM_ERR_CAPACITY;
      n = pmax;
    }
    n_path[k] = n;
    for (int i = 0; i < pmax; ++i)
      for (int c = 0; c < 3; ++c) path[((size_t)k * pmax + i) * 3 + c] = i < n ? pl[i][c] : pl[n - 1][c];
  }
  return HDSM_OK;
}

int hdsm_swarm_reference_inputs(void* swarm, double* path, int32_t* n_path) {
  return hdsm_swarm_reference_inputs_n(swarm, 3, path, n_path);
}

int hdsm_swarm_vel_cap(void* swarm, double* vel_cap) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !vel_cap) return HDSM_ERR_BAD_ARG;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  const hdsm_ref_config rc = ref_config(*sw);
  for (int k = 0; k < sw->n_local; ++k) {
    const AgentS& ag = sw->agents[k];
    V3 pl[hdsm_sw::PATH_PTS + 1];
    const int n = hdsm_sw::reference_polyline(ag, pl);
    vel_cap[k] = hdsm_sw::voxel_velocity_cap(cc, rc, hdsm_sw::local_grid_origin(cc, ag), pl, n);
  }
  return HDSM_OK;
}

int hdsm_swarm_set_reference(void* swarm, const double* ref_full, const double* path_vel) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !ref_full || !path_vel) return HDSM_ERR_BAD_ARG;
  const int N = sw->prm.n_hor;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  for (int k = 0; k < sw->n_local; ++k) {
    AgentS& ag = sw->agents[k];
    ag.n_ref = N + 1;
    for (int i = 0; i <= N; ++i)
      for (int c = 0; c < 6; ++c) ag.traj_ref[i][c] = ref_full[((size_t)k * (N + 1) + i) * 6 + c];
    ag.path_vel = path_vel[k];
    ag.external_ref = 1;
    hdsm_sw::keep_only_free(cc, hdsm_sw::local_grid_origin(cc, ag), ag.path_vel, ag.traj_ref, ag.n_ref);  // AC:1512-1514
  }
  return HDSM_OK;
}

int hdsm_swarm_state(void* swarm, double* pos, double* dist_goal, int32_t* n_fail) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k) {
    const AgentS& ag = sw->agents[k];
    const V3 p = {{ag.state_curr[0], ag.state_curr[1], ag.state_curr[2]}};
    if (pos)
      for (int c = 0; c < 3; ++c) pos[3 * k + c] = p[c];
    if (dist_goal) dist_goal[k] = norm(sub(p, ag.goal));
    if (n_fail) n_fail[k] = ag.n_fail;
  }
  return HDSM_OK;
}

int hdsm_swarm_yaw(void* swarm, int32_t yaw_idx, double k_p_yaw, double* yaw_out) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || yaw_idx < 0 || yaw_idx > sw->prm.n_hor) return HDSM_ERR_BAD_ARG;
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < sw->n_local; ++k) {
    const AgentS& ag = sw->agents[k];
    double& yaw = sw->extra[k].yaw;
    if (ag.n_ref > yaw_idx) {  // AC:1028-1030 (traj_ref_curr_ exists from the first reference on)
      double v[3] = {ag.traj_ref[yaw_idx][0] - ag.state_curr[0], ag.traj_ref[yaw_idx][1] - ag.state_curr[1], ag.traj_ref[yaw_idx][2] - ag.state_curr[2]};
      if (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] > 0.1) {  // AC:1033
        const double yaw_ref = std::atan2(v[1], v[0]);        // AC:1035-1040 (the projection on the x-y plane drops v[2])
        double error_ang = yaw_ref - yaw;
        if (error_ang > pi) error_ang = error_ang - 2 * pi;  // AC:1043-1047
        else if (error_ang < -pi) error_ang = error_ang + 2 * pi;
        yaw = yaw + k_p_yaw * error_ang * sw->prm.dt;         // AC:1048
      }
    }
    if (yaw_out) yaw_out[k] = yaw;
  }
  return HDSM_OK;
}

// Test hook (tests/test_host.py; not in include/): the minimum distance of the samples of the increment check (AC:569-585) to `pt`,
// per segment, from the literal 1-cm walk and from the closed form the device's k_commit tries first. ref [n_ref][3].
int hdsm_internal_increment_minima(const double* ref, int32_t n_ref, const double* pt, double* literal, double* closed_form) {
  if (!ref || !pt || n_ref < 2 || n_ref > hdsm::MAXH + 1) return HDSM_ERR_BAD_ARG;
  static thread_local AgentS ag;
  ag.n_ref = n_ref;
  for (int i = 0; i < n_ref; ++i)
    for (int k = 0; k < 3; ++k) ag.traj_ref[i][k] = ref[3 * i + k];
  const hdsm_sw::V3 p = {{pt[0], pt[1], pt[2]}};
  for (int seg = 0; seg + 1 < n_ref; ++seg) {
    if (literal) literal[seg] = hdsm_sw::increment_segment_min(ag, seg, p);
    if (closed_form) closed_form[seg] = hdsm_sw::increment_segment_min_closed_form(ag, seg, p);
  }
  return HDSM_OK;
}

int hdsm_swarm_view(void* swarm, int32_t k, double* traj_curr, int32_t* n_traj, double* traj_ref, int32_t* n_ref, double* path, int32_t pmax,
                    int32_t* n_path, int32_t* n_poly, int32_t* poly_rows, double* poly_A, double* poly_b, double* poly_seeds, double pos[3]) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || k < 0 || k >= sw->n_local) return HDSM_ERR_BAD_ARG;
  const AgentS& ag = sw->agents[k];
  const int N = sw->prm.n_hor, P = sw->prm.poly_hor, RS = sw->prm.max_rows_static;
  const int nt = ag.has_traj ? N + 1 : 0, nr = ag.n_ref < N + 1 ? ag.n_ref : N + 1;
  if (n_traj) *n_traj = nt;
  if (traj_curr)
    for (int i = 0; i < nt; ++i)
      for (int c = 0; c < 3; ++c) traj_curr[3 * i + c] = ag.traj_curr[i][c];
  if (n_ref) *n_ref = nr;
  if (traj_ref)
    for (int i = 0; i < nr; ++i)
      for (int c = 0; c < 3; ++c) traj_ref[3 * i + c] = ag.traj_ref[i][c];
  const int np = ag.n_path < pmax ? ag.n_path : pmax;
  if (n_path) *n_path = np;
  if (path)
    for (int i = 0; i < np; ++i)
      for (int c = 0; c < 3; ++c) path[3 * i + c] = ag.path[i][c];
  const int npl = ag.n_poly < P ? ag.n_poly : P;
  if (n_poly) *n_poly = npl;
  for (int j = 0; j < npl; ++j) {
    const hdsm_sw::Poly& pl = ag.polys[j];
    const int rows = pl.rows < RS ? pl.rows : RS;
    if (poly_rows) poly_rows[j] = rows;
    for (int r = 0; r < rows; ++r) {
      if (poly_A)
        for (int c = 0; c < 3; ++c) poly_A[((size_t)j * RS + r) * 3 + c] = pl.A[r][c];
      if (poly_b) poly_b[(size_t)j * RS + r] = pl.b[r];
    }
    if (poly_seeds)
      for (int c = 0; c < 3; ++c) poly_seeds[3 * j + c] = pl.seed[c];
  }
  if (pos)
    for (int c = 0; c < 3; ++c) pos[c] = ag.state_curr[c];
  return HDSM_OK;
}

}  // extern "C"
