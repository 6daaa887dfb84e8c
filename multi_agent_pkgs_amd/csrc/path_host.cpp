// path_host.cpp — the host form of the path step (path_core.h): hdsm_local_path_host and the planner the host mirror calls
// (hdsm_swarm_replan_paths, the path period, hdsm_swarm_set_goals). Pure host C++.
#include <cmath>
#include <cstring>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/hdsm_swarm.h"
#include "hdsm_internal.h"
#include "path_core.h"

namespace hdsm_path {

// steps 1-6 of path_core.h with a queue BFS over a dense level array (levels are unique: the same field as the device's
// level-synchronous search, which only keeps them mod 3): the descent's voxels (x + dx (y + dy z)), start voxel first
static int prior_chain(const PathIn& in, Ends* e, std::vector<int32_t>* chain) {
  const int st = path_setup(in, e);
  if (st != PATH_OK) return st;
  const int dx = in.g.dim[0], dy = in.g.dim[1], dz = in.g.dim[2];
  auto id = [&](int i, int j, int k) { return i + dx * (j + dy * k); };
  thread_local std::vector<int32_t> level, queue;
  level.assign((size_t)dx * dy * dz, -1);
  queue.resize((size_t)dx * dy * dz);
  const int sid = id(e->sv[0], e->sv[1], e->sv[2]), gid = id(e->gv[0], e->gv[1], e->gv[2]);
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
  chain->clear();
  chain->reserve((size_t)L + 1);
  int v[3] = {e->sv[0], e->sv[1], e->sv[2]};
  chain->push_back(sid);
  auto code = [&](int i, int j, int k) { return level[id(i, j, k)]; };
  for (int lv = L; lv > 0; --lv) {
    if (!descend_step(in.g, v, lv - 1, code)) return PATH_UNREACHABLE;
    chain->push_back(id(v[0], v[1], v[2]));
  }
  return PATH_OK;
}

static V3 centre_of(const PathIn& in, int id) {
  const int dx = in.g.dim[0], dy = in.g.dim[1];
  return centre(in, id % dx, (id / dx) % dy, id / (dx * dy));
}

// steps 1-7 of path_core.h
int plan_serial(const PathIn& in, V3* out, int* n_out) {
  if (in.g.world == nullptr) return free_space_path(in, out, n_out);
  Ends e;
  std::vector<int32_t> chain;
  const int st = prior_chain(in, &e, &chain);
  if (st != PATH_OK) return st;
  std::vector<V3> q;
  q.reserve(chain.size() + 1);
  q.push_back(in.start);
  for (size_t t = 1; t + 1 < chain.size(); ++t) q.push_back(centre_of(in, chain[t]));
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

// 6b: the mask of DMPlanner::setPath, literally (libm's hypot in double decides the points on the sphere)
bool dmp_build_mask(double search_rad, double res, DmpMask* mask) {
  std::memset(mask->rows, 0, sizeof mask->rows);
  if (search_rad < 0) {
    mask->rn = -1;
    return true;
  }
  const int rn = (int)std::ceil(search_rad / res), hn = rn;
  mask->rn = rn;
  if (rn > DMP_MAX_RN) return false;
  const int R = 2 * rn + 1;
  for (int nx = -rn; nx <= rn; ++nx)
    for (int ny = -rn; ny <= rn; ++ny)
      for (int nz = -hn; nz <= hn; ++nz) {
        if (std::hypot(std::hypot(nx, ny), nz) > rn) continue;
        mask->rows[(nz + rn) * R + (ny + rn)] |= 1u << (nx + rn);
      }
  return true;
}

// steps 1-6, 6a-7' of path_core.h: a heap Dijkstra from the goal voxel until the start voxel is settled (every voxel the descent
// can compare against has a smaller D and is settled by then; an unsettled voxel's tentative value is not below D(sv))
int plan_dmp_serial(const PathIn& in, const DmpMask& mask, V3* out, int* n_out, int* cost_out, int* n_raw_out) {
  *cost_out = -1, *n_raw_out = 0, *n_out = 0;
  if (in.g.world == nullptr) {
    *cost_out = 0;
    return free_space_path(in, out, n_out);
  }
  if (mask.rn > DMP_MAX_RN) return PATH_WORKSPACE;
  Ends e;
  std::vector<int32_t> prior;
  int st = prior_chain(in, &e, &prior);
  if (st != PATH_OK) return st;
  const int dx = in.g.dim[0], dy = in.g.dim[1], dz = in.g.dim[2], rn = mask.rn;
  const DmpGrid dg{in.g};
  auto id = [&](int i, int j, int k) { return i + dx * (j + dy * k); };
  thread_local std::vector<uint8_t> in_t;
  thread_local std::vector<int32_t> D;
  const size_t nvox = (size_t)dx * dy * dz;
  in_t.assign(nvox, 0);
  long long nt = 0;
  if (rn < 0) {
    for (int k = 0; k < dz; ++k)
      for (int j = 0; j < dy; ++j)
        for (int i = 0; i < dx; ++i)
          if (!in.g.occupied(i, j, k)) in_t[id(i, j, k)] = 1, ++nt;
  } else {
    const int R = 2 * rn + 1;
    for (int32_t pv : prior) {
      const int pi = pv % dx, pj = (pv / dx) % dy, pk = pv / (dx * dy);
      for (int nz = -rn; nz <= rn; ++nz)
        for (int ny = -rn; ny <= rn; ++ny) {
          const uint32_t m = mask.rows[(nz + rn) * R + (ny + rn)];
          for (int nx = -rn; m != 0u && nx <= rn; ++nx) {
            const int i = pi + nx, j = pj + ny, k = pk + nz;
            if (!((m >> (nx + rn)) & 1u) || !in.g.inside(i, j, k) || in_t[id(i, j, k)] || in.g.occupied(i, j, k)) continue;
            in_t[id(i, j, k)] = 1, ++nt;
          }
        }
    }
  }
  if (nt > DMP_FIELD) return PATH_WORKSPACE;
  const int32_t INF = 0x7fffffff;
  D.assign(nvox, INF);
  const int sid = id(e.sv[0], e.sv[1], e.sv[2]), gid = id(e.gv[0], e.gv[1], e.gv[2]);
  auto cost_of = [&](int v) { return dg.cost(v % dx, (v / dx) % dy, v / (dx * dy)); };
  typedef std::pair<int32_t, int32_t> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  D[gid] = cost_of(gid);
  heap.push(Item(D[gid], gid));
  bool found = false;
  while (!heap.empty()) {
    const Item top = heap.top();
    heap.pop();
    const int v = top.second;
    if (top.first != D[v]) continue;
    if (v == sid) {
      found = true;
      break;
    }
    const int k = v / (dx * dy), j = (v / dx) % dy, i = v % dx;
    const int nb[6][3] = {{i - 1, j, k}, {i + 1, j, k}, {i, j - 1, k}, {i, j + 1, k}, {i, j, k - 1}, {i, j, k + 1}};
    for (const auto& n : nb) {
      if (!in.g.inside(n[0], n[1], n[2])) continue;
      const int w = id(n[0], n[1], n[2]);
      if (!in_t[w]) continue;
      const int32_t d = top.first + 1 + cost_of(w);
      if (d < D[w]) D[w] = d, heap.push(Item(d, w));
    }
  }
  if (!found) return PATH_UNREACHABLE;  // (cannot happen: the prior chain lies in T)
  // 6d
  std::vector<int32_t> chain;
  chain.push_back(sid);
  int v[3] = {e.sv[0], e.sv[1], e.sv[2]}, cur = sid;
  while (cur != gid) {
    const int want = D[cur] - 1 - cost_of(cur);
    auto code = [&](int i, int j, int k) { return in_t[id(i, j, k)] ? D[id(i, j, k)] : INF; };
    if (want < 0 || !descend_step(in.g, v, want, code)) return PATH_UNREACHABLE;
    if ((int)chain.size() == MAX_DESCENT) return PATH_WORKSPACE;
    cur = id(v[0], v[1], v[2]);
    chain.push_back(cur);
  }
  // 6e
  std::vector<V3> q;
  q.reserve(chain.size() + 2);
  q.push_back(in.start);
  for (int32_t c : chain) q.push_back(centre_of(in, c));
  if (!goal_moved(in, e)) q.push_back(e.gq);
  // 7': ShortenDMPPath's walk. After its erase the point at i_start + 1 is the old i_end, which is where i goes next: so the walk
  // is over indices of the unshortened path, and the points it stands on are the output
  const int npts = (int)q.size();
  int a = 0, n = 0;
  for (;;) {
    if (n == PATH_PTS) return PATH_TOO_LONG;
    out[n++] = q[a];
    if (a >= npts - 1) break;
    int next = a + 1;
    const V3 la = to_local(in, q[a]);
    if (dg.at(la) <= 0) {
      int i_end = a;
      for (int j = a + 1; j < npts && dmp_segment_ok(dg, la, to_local(in, q[j])); ++j) i_end = j;
      if (i_end > a) next = i_end;
    }
    a = next;
  }
  *n_out = n, *cost_out = D[sid], *n_raw_out = (int)chain.size();
  return PATH_OK;
}

}  // namespace hdsm_path

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

extern "C" int hdsm_local_path_dmp_host(int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                                        const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res,
                                        double search_rad, int32_t pmax, double* paths, int32_t* n_path, int32_t* status, int32_t* cost,
                                        int32_t* n_raw) {
  if (n < 0 || !ldim || !off || !ground_k || !origin || !start || !goal || !(res > 0) || !(search_rad == search_rad) || pmax < 2 || !paths ||
      !n_path || !status || !cost || !n_raw || (world && !wdim))
    return HDSM_ERR_BAD_ARG;
  hdsm_path::DmpMask mask;
  hdsm_path::dmp_build_mask(search_rad, res, &mask);  // (a radius over DMP_MAX_RN voxels: status 4 for every case in a world)
  int rc = HDSM_OK;
  for (int t = 0; t < n; ++t) {
    hdsm_path::PathIn in;
    hdsm_internal_path_case(t, world, wdim, ldim, off, ground_k, origin, start, goal, res, &in);
    hdsm_sw::V3 out[hdsm_sw::PATH_PTS];
    int np = 0, c = -1, nr = 0;
    status[t] = hdsm_path::plan_dmp_serial(in, mask, out, &np, &c, &nr);
    if (status[t] != hdsm_path::PATH_OK) np = 0, c = -1, nr = 0;
    n_path[t] = np, cost[t] = c, n_raw[t] = nr;
    if (np > pmax) rc = HDSM_ERR_CAPACITY;
    for (int i = 0; i < pmax; ++i)
      for (int k = 0; k < 3; ++k) paths[((size_t)t * pmax + i) * 3 + k] = np ? out[i < np ? i : np - 1][k] : 0.0;
  }
  return rc;
}
