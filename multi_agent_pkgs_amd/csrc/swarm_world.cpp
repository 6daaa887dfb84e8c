// swarm_world.cpp — the host mirror's world and global paths between rounds (include/hdsm_swarm.h): the world and its map updates,
// paths and goals, the path step's period and clearance mode, and the path step itself. Pure host C++.
#include <cmath>
#include <cstring>

#include "swarm_host.h"

using namespace hdsm_mirror;

// Agent::UpdatePath (AC:261-454) for one agent, the rule of path_core.h: on success the new path replaces path_curr_, on failure
// the agent keeps its path; the status stays in ag.path_rc (hdsm_swarm_path_errors)
// (dmp: the tunnel's mask in clearance mode, else NULL)
int hdsm_mirror::replan_agent(const hdsm_sw::Cfg& cc, AgentS& ag, const hdsm_path::DmpMask* dmp) {
  V3 out[hdsm_sw::PATH_PTS];
  int n = 0, cost = 0, n_raw = 0;
  const hdsm_path::PathIn in = hdsm_path::agent_problem(cc, ag, ag.goal);
  const int st = dmp ? hdsm_path::plan_dmp_serial(in, *dmp, out, &n, &cost, &n_raw) : hdsm_path::plan_serial(in, out, &n);
  ag.path_rc = st;
  if (st == hdsm_path::PATH_OK) {
    ag.n_path = n;
    for (int i = 0; i < n; ++i) ag.path[i] = out[i];
  }
  return st;
}

// the path step at the start of a round, before the corridor (the device loop's k_path does the same in the same rounds)
void hdsm_mirror::path_round(Swarm& sw, const hdsm_sw::Cfg& cc) {
  PathStep& p = sw.path;
  const bool all = p.period > 0 && p.round % p.period == 0;
  for (int k = 0; k < sw.n_local; ++k)
    if (all || p.due[k]) {
      replan_agent(cc, sw.agents[k], p.dmp());
      p.due[k] = 0;
    }
  ++p.round;
}

// the agents whose status `rc` is not 0; the statuses into codes [n_local] (may be NULL)
static int count_errors(void* swarm, int32_t AgentS::*rc, int32_t* codes) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  int n = 0;
  for (int k = 0; k < sw->n_local; ++k) {
    if (codes) codes[k] = sw->agents[k].*rc;
    n += sw->agents[k].*rc != 0;
  }
  return n;
}

extern "C" {

int hdsm_swarm_set_world(void* swarm, const int8_t* occupancy, const int32_t dim[3], const double origin[3]) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !dim || !origin) return HDSM_ERR_BAD_ARG;
  World& w = sw->world;
  if (!occupancy) {
    w.has = false;
    w.grid.clear();
    return HDSM_OK;
  }
  if (dim[0] < 1 || dim[1] < 1 || dim[2] < 1) return HDSM_ERR_BAD_ARG;
  for (int ax = 0; ax < 3; ++ax) {  // local grids must register with the world grid
    const double q = origin[ax] / sw->cfg.voxel_size;
    if (std::fabs(q - std::round(q)) > 1e-9) return HDSM_ERR_BAD_ARG;
    w.dim[ax] = dim[ax], w.origin[ax] = origin[ax];
  }
  w.grid.assign(occupancy, occupancy + (size_t)dim[0] * dim[1] * dim[2]);
  w.has = true;
  return HDSM_OK;
}

// A map update (VoxelGridResponseCallback / MappingUtilVoxelGridCallback, AC:2310-2378, for the shared world): the box lo .. lo + bdim
// of the processed world takes `values` [bdim[2]][bdim[1]][bdim[0]] as they are. Everything reads the world at the moment it runs, so
// the next corridor / path step sees the new voxels as after hdsm_swarm_set_world of the edited grid; kept polyhedra are not looked at
// again (AC:1253-1282 keeps them too).
int hdsm_swarm_update_world(void* swarm, const int8_t* values, const int32_t lo[3], const int32_t bdim[3]) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->world.has || !lo || !bdim) return HDSM_ERR_BAD_ARG;
  World& w = sw->world;
  for (int ax = 0; ax < 3; ++ax)
    if (bdim[ax] < 0 || lo[ax] < 0 || lo[ax] > w.dim[ax] || bdim[ax] > w.dim[ax] - lo[ax]) return HDSM_ERR_BAD_ARG;
  if (bdim[0] == 0 || bdim[1] == 0 || bdim[2] == 0) return HDSM_OK;
  if (!values) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < bdim[2]; ++k)
    for (int j = 0; j < bdim[1]; ++j)
      std::memcpy(&w.grid[((size_t)(lo[2] + k) * w.dim[1] + (lo[1] + j)) * w.dim[0] + lo[0]], values + ((size_t)k * bdim[1] + j) * bdim[0],
                  (size_t)bdim[0]);
  return HDSM_OK;
}

int hdsm_swarm_set_paths(void* swarm, const double* paths, const int32_t* n_path, int32_t pmax) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !paths || !n_path || pmax < 2) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k)
    if (n_path[k] < 2 || n_path[k] > pmax || n_path[k] > hdsm_sw::PATH_PTS) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k) {
    AgentS& ag = sw->agents[k];
    ag.n_path = n_path[k];
    for (int i = 0; i < n_path[k]; ++i) {
      const double* p = paths + ((size_t)k * pmax + i) * 3;
      ag.path[i] = V3{{p[0], p[1], p[2]}};
    }
  }
  return HDSM_OK;
}

int hdsm_swarm_get_paths(void* swarm, int32_t pmax, double* paths, int32_t* n_path) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !paths || !n_path || pmax < 2) return HDSM_ERR_BAD_ARG;
  int rc = HDSM_OK;
  for (int k = 0; k < sw->n_local; ++k) {
    const AgentS& ag = sw->agents[k];
    n_path[k] = ag.n_path;
    if (ag.n_path > pmax) rc = HDSM_ERR_CAPACITY;
    for (int i = 0; i < pmax; ++i) {
      const V3& p = ag.path[i < ag.n_path ? i : ag.n_path - 1];
      for (int c = 0; c < 3; ++c) paths[((size_t)k * pmax + i) * 3 + c] = p[c];
    }
  }
  return rc;
}

int hdsm_swarm_set_goals(void* swarm, const double* goals) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || (!goals && sw->n_local)) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < sw->n_local; ++k) {
    AgentS& ag = sw->agents[k];
    const double* g = goals + 3 * (size_t)k;
    if (g[0] == ag.goal[0] && g[1] == ag.goal[1] && g[2] == ag.goal[2]) continue;
    ag.goal = V3{{g[0], g[1], g[2]}};
    sw->path.due[k] = 1;
  }
  return HDSM_OK;
}

int hdsm_swarm_set_path_period(void* swarm, int32_t period) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || period < 0) return HDSM_ERR_BAD_ARG;
  sw->path.period = period;
  sw->path.round = 0;  // (the next round is due)
  return HDSM_OK;
}

int hdsm_swarm_set_path_clearance(void* swarm, double search_rad) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !(search_rad == search_rad)) return HDSM_ERR_BAD_ARG;
  hdsm_path::DmpMask mask{};
  if (search_rad != 0 && !hdsm_path::dmp_build_mask(search_rad, sw->cfg.voxel_size, &mask)) return HDSM_ERR_BAD_ARG;  // over DMP_MAX_RN voxels
  sw->path.clearance = search_rad, sw->path.mask = mask;
  return HDSM_OK;
}

int hdsm_swarm_replan_paths(void* swarm, int32_t* n_failed) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  const hdsm_sw::Cfg cc = sw->core_cfg();
  int failed = 0;
  for (int k = 0; k < sw->n_local; ++k) failed += replan_agent(cc, sw->agents[k], sw->path.dmp()) != hdsm_path::PATH_OK;
  if (n_failed) *n_failed = failed;
  return HDSM_OK;
}

int hdsm_swarm_path_errors(void* swarm, int32_t* codes) { return count_errors(swarm, &AgentS::path_rc, codes); }

int hdsm_swarm_corridor_errors(void* swarm, int32_t* codes) { return count_errors(swarm, &AgentS::corridor_rc, codes); }

}  // extern "C"
