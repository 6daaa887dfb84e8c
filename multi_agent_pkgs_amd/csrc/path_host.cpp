// path_host.cpp — the host form of the path step (path_core.h): hdsm_local_path_host and the planner the host mirror calls
// (hdsm_swarm_replan_paths, the path period, hdsm_swarm_set_goals). Pure host C++.
#include <cstring>
#include <vector>

#include "../../include/hdsm_swarm.h"
#include "path_core.h"

namespace hdsm_path {

// steps 1-7 of path_core.h with a queue BFS over a dense level array (levels are unique: the same field as the device's
// level-synchronous search, which only keeps them mod 3)
int plan_serial(const PathIn& in, V3* out, int* n_out) {
  if (in.g.world == nullptr) return free_space_path(in, out, n_out);
  Ends e;
  const int st = path_setup(in, &e);
  if (st != PATH_OK) return st;
  const int dx = in.g.dim[0], dy = in.g.dim[1], dz = in.g.dim[2];
  auto id = [&](int i, int j, int k) { return i + dx * (j + dy * k); };
  thread_local std::vector<int32_t> level, queue;
  level.assign((size_t)dx * dy * dz, -1);
  queue.resize((size_t)dx * dy * dz);
  const int sid = id(e.sv[0], e.sv[1], e.sv[2]), gid = id(e.gv[0], e.gv[1], e.gv[2]);
  size_t head = 0, tail = 0;
  level[gid] = 0;
  queue[tail++] = gid;
  while (level[sid] < 0 && head < tail) {  // stops as soon as the start voxel has a level
    const int v = queue[head++], k = v / (dx * dy), j = (v / dx) % dy, i = v % dx;
    const int nb[6][3] = {{i - 1, j, k}, {i + 1, j, k}, {i, j - 1, k}, {i, j + 1, k}, {i, j, k - 1}, {i, j, k + 1}};
    for (const auto& n : nb) {
      if (in.g.blocked(n[0], n[1], n[2])) continue;
      const int w = id(n[0], n[1], n[2]);
      if (level[w] >= 0) continue;
      level[w] = level[v] + 1;
      queue[tail++] = w;
    }
  }
  if (level[sid] < 0) return PATH_UNREACHABLE;
  const int L = level[sid];
  if (L + 1 > MAX_DESCENT) return PATH_WORKSPACE;
  std::vector<V3> q;
  q.reserve((size_t)L + 2);
  q.push_back(in.start);
  int v[3] = {e.sv[0], e.sv[1], e.sv[2]};
  auto code = [&](int i, int j, int k) { return level[id(i, j, k)]; };
  for (int lv = L; lv > 1; --lv) {
    if (!descend_step(in.g, v, lv - 1, code)) return PATH_UNREACHABLE;
    q.push_back(centre(in, v[0], v[1], v[2]));
  }
  q.push_back(e.gq);  // (start voxel = goal voxel: [S, G])
  const int m = (int)q.size() - 1;
  int a = 0, n = 1;
  out[0] = q[0];
  while (a < m) {
    int j = a + 1;
    for (int c = m; c > a + 1; --c)
      if (segment_clear(in, q[a], q[c])) {
        j = c;
        break;
      }
    if (n == PATH_PTS) return PATH_TOO_LONG;
    out[n++] = q[j];
    a = j;
  }
  *n_out = n;
  return PATH_OK;
}

}  // namespace hdsm_path

// the argument checks and the per-case problem of hdsm_local_path_host / hdsm_local_path_batch
extern "C" int hdsm_internal_path_case(int32_t t, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                                       const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res,
                                       void* problem) {
  hdsm_path::PathIn& in = *static_cast<hdsm_path::PathIn*>(problem);
  in.g.world = world;
  for (int ax = 0; ax < 3; ++ax) {
    in.g.wdim[ax] = world ? wdim[ax] : 0, in.g.dim[ax] = ldim[ax], in.g.off[ax] = off[3 * (size_t)t + ax];
    in.origin[ax] = origin[3 * (size_t)t + ax], in.start[ax] = start[3 * (size_t)t + ax], in.goal[ax] = goal[3 * (size_t)t + ax];
  }
  in.g.ground_k = ground_k[t];
  in.res = res;
  return HDSM_OK;
}

extern "C" int hdsm_local_path_host(int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                                    const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res,
                                    int32_t pmax, double* paths, int32_t* n_path, int32_t* status) {
  if (n < 0 || !ldim || !off || !ground_k || !origin || !start || !goal || !(res > 0) || pmax < 2 || !paths || !n_path || !status ||
      (world && !wdim))
    return HDSM_ERR_BAD_ARG;
  int rc = HDSM_OK;
  for (int t = 0; t < n; ++t) {
    hdsm_path::PathIn in;
    hdsm_internal_path_case(t, world, wdim, ldim, off, ground_k, origin, start, goal, res, &in);
    hdsm_sw::V3 out[hdsm_sw::PATH_PTS];
    int np = 0;
    status[t] = hdsm_path::plan_serial(in, out, &np);
    if (status[t] != hdsm_path::PATH_OK) np = 0;
    n_path[t] = np;
    if (np > pmax) rc = HDSM_ERR_CAPACITY;
    for (int i = 0; i < pmax; ++i)
      for (int c = 0; c < 3; ++c) paths[((size_t)t * pmax + i) * 3 + c] = np ? out[i < np ? i : np - 1][c] : 0.0;
  }
  return rc;
}
