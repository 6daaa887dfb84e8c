// path_core.h — the path step of Agent::UpdatePath (AC:261-454) for one agent, as plain functions that compile for the host form
// (path_host.cpp: hdsm_local_path_host, the host mirror's hdsm_swarm_replan_paths / path period) AND for the device (k_path / k_dmp in
// swarm_kernels.hip, k_path_batch / k_dmp_batch in path_kernels.hip): one source for the grid, the goal, the start, the descent and the
// shortening, so the two give the same points bit for bit. AC = multi_agent_planner/src/agent_class.cpp of the reference.
//
// NOT the reference's planner: UpdatePath runs JPS3D + a distance-map planner (DMP) and ShortenDMPPath. By default this is a stated
// stand-in for all three (the clearance mode further down keeps the descent as the stand-in for JPS only and reproduces the DMP and
// ShortenDMPPath), like the host router of hdsm_swarm_route — a breadth-first search on the same local grid with a greedy
// line-of-sight shortening. What it keeps of the reference: the grid (the agent's local grid as a window of the world,
// ClearBoundary AC:1819-1854), the start (where the kept reference ends, AC:328-350), the goal (GetIntermediateGoal
// AC:1891-1941) and the line-of-sight test (the Raycast of swarm_core.h). For one agent:
//   1 grid     local grid at local_grid_origin; unknown world voxels and voxels below ground_k occupied, outside the world free,
//              >= 100 occupied (1..99, the potential field, free); then ClearBoundary: the x and y side faces free
//   2 start    S = the point reference_polyline starts from this round (traj_ref[1] / traj_ref[0] / path[0])
//   3 goal     G = GetIntermediateGoal(goal)
//   4 voxels   an occupied (or outside) start / goal voxel is replaced by the nearest free one: Chebyshev shells r = 1..6,
//              smallest squared offset, first in dk, dj, di ascending order; none -> status 1
//   5 search   6-connected unit-cost BFS from the goal voxel until the start voxel has a level; never -> status 2
//   6 descent  from the start voxel, each step to the first neighbour (-x, +x, -y, +y, -z, +z) one level lower; candidates
//              q0 = S, q1..q(m-1) voxel centres, qm = G (or the goal voxel's centre if step 4 moved it)
//   7 shorten  from a = 0 the largest j > a with a clear segment q_a -> q_j (j = a + 1 always accepted); > PATH_PTS -> status 3
// No world: path = [S, goal]. Status 4: the local grid (padded by one voxel in x and y) or the descent does not fit the
// device's workspace (PLANE_WORDS); the host form applies the same limit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "swarm_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_path {

using hdsm_sw::AgentS;
using hdsm_sw::Cfg;
using hdsm_sw::V3;
using hdsm_sw::PATH_PTS;

enum { PATH_OK = 0, PATH_NO_FREE_VOXEL = 1, PATH_UNREACHABLE = 2, PATH_TOO_LONG = 3, PATH_WORKSPACE = 4 };

constexpr int SHELLS = 6;            // nearest-free search radius (voxels), the router's
constexpr int PLANE_WORDS = 6144;    // device: one bit plane of the padded local grid (dx + 2)(dy + 2) dz <= 196608 bits
                                     // (66 x 66 x 40: the 12 m high grid of cfg 5)
constexpr int MAX_DESCENT = PLANE_WORDS;  // voxels of a descent (device: kept in the blocked plane after the search)
constexpr int THREADS = 512;         // device: threads of a workgroup that plans one agent

// The occupancy predicate of step 1, on the agent's local grid (window of the world, x fastest)
struct PathGrid {
  const int8_t* world;
  int wdim[3], dim[3], off[3], ground_k;
  CD_HD bool inside(int i, int j, int k) const { return i >= 0 && j >= 0 && k >= 0 && i < dim[0] && j < dim[1] && k < dim[2]; }
  CD_HD bool occupied(int i, int j, int k) const {  // (i, j, k) inside the grid
    if (i == 0 || j == 0 || i == dim[0] - 1 || j == dim[1] - 1) return false;  // ClearBoundary, AC:1819-1854 (not floor / roof)
    if (k < ground_k) return true;
    const int gi = i + off[0], gj = j + off[1], gk = k + off[2];
    if (gi < 0 || gj < 0 || gk < 0 || gi >= wdim[0] || gj >= wdim[1] || gk >= wdim[2]) return false;
    const int v = world[(size_t)gi + (size_t)gj * wdim[0] + (size_t)gk * wdim[0] * wdim[1]];
    return v < 0 || v >= 100;
  }
  CD_HD bool blocked(int i, int j, int k) const { return !inside(i, j, k) || occupied(i, j, k); }
  CD_HD int value(int i, int j, int k) const { return occupied(i, j, k) ? 100 : 0; }  // what raycast tests
};

struct PathIn {
  PathGrid g;
  V3 origin, start, goal;
  double res;
};

// the problem of one agent of a swarm this round: its local grid, the start of its reference polyline, its goal
CD_HD PathIn agent_problem(const Cfg& c, const AgentS& ag, const V3& goal) {
  PathIn in;
  in.origin = hdsm_sw::local_grid_origin(c, ag);
  const hdsm_sw::RawWindow w = hdsm_sw::raw_window(c, in.origin);
  in.g.world = c.has_world ? c.world : nullptr;
  for (int ax = 0; ax < 3; ++ax) in.g.wdim[ax] = c.wdim[ax], in.g.dim[ax] = w.dim[ax], in.g.off[ax] = w.off[ax];
  in.g.ground_k = w.ground_k;
  in.res = c.voxel_size;
  if (ag.n_ref > 0) {  // reference_polyline's starting point (AC:1459-1478)
    const double* r = ag.increment ? ag.traj_ref[1] : ag.traj_ref[0];
    in.start = {{r[0], r[1], r[2]}};
  } else {
    in.start = ag.path[0];
  }
  in.goal = goal;
  return in;
}

// GetIntermediateGoal, AC:1891-1941, statement by statement (the reference's march never counts n_it up; here it stops after
// 100 half-voxel steps, which leaves any grid of up to 50 voxels beyond the sampled start)
CD_HD V3 intermediate_goal(const V3& goal, const V3& origin, const int dim[3], double vs) {
  V3 g;
  for (int ax = 0; ax < 3; ++ax) g[ax] = goal[ax] - origin[ax];
  const double dr[3] = {dim[0] * vs, dim[1] * vs, dim[2] * vs};
  if (g[0] < dr[0] && g[0] > 0 && g[1] < dr[1] && g[1] > 0 && g[2] < dr[2] && g[2] > 0) return goal;
  const V3 centre = {{(dim[0] / 2 + 0.5) * vs, (dim[1] / 2 + 0.5) * vs, (dim[2] / 2 + 0.5) * vs}};
  V3 dir = {{g[0] - centre[0], g[1] - centre[1], g[2] - centre[2]}};
  const double z = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];  // Eigen normalize(): /= sqrt(squaredNorm) if > 0
  if (z > 0) {
    const double s = sqrt(z);
    for (int ax = 0; ax < 3; ++ax) dir[ax] = dir[ax] / s;
  }
  const int dmin = dim[0] < dim[1] ? (dim[0] < dim[2] ? dim[0] : dim[2]) : (dim[1] < dim[2] ? dim[1] : dim[2]);
  const double min_dim = vs * dmin;
  V3 p;
  for (int ax = 0; ax < 3; ++ax) p[ax] = centre[ax] + (min_dim / 2) * dir[ax];
  const double half = 0.5 * vs;
  for (int n_it = 0; n_it < 100; ++n_it) {
    if (p[0] > dr[0] || p[1] > dr[1] || p[2] > dr[2] || p[0] < 0 || p[1] < 0 || p[2] < 0) {
      for (int ax = 0; ax < 3; ++ax) p[ax] = p[ax] - half * dir[ax];
      break;
    }
    for (int ax = 0; ax < 3; ++ax) p[ax] = p[ax] + half * dir[ax];
  }
  return {{p[0] + origin[0], p[1] + origin[1], p[2] + origin[2]}};
}

CD_HD void voxel_of(const PathIn& in, const V3& p, int v[3]) {
  for (int ax = 0; ax < 3; ++ax) v[ax] = (int)floor((p[ax] - in.origin[ax]) / in.res);
}
CD_HD V3 centre(const PathIn& in, int i, int j, int k) {
  return {{in.origin[0] + (i + 0.5) * in.res, in.origin[1] + (j + 0.5) * in.res, in.origin[2] + (k + 0.5) * in.res}};
}

// step 4: the router's rule (hdsm_swarm_route's nearest_free) on the local grid; outside the grid counts as blocked
CD_HD bool nearest_free(const PathGrid& g, int v[3]) {
  if (!g.blocked(v[0], v[1], v[2])) return true;
  for (int r = 1; r <= SHELLS; ++r) {
    int best = 1 << 30, bv[3] = {0, 0, 0};
    for (int dk = -r; dk <= r; ++dk)
      for (int dj = -r; dj <= r; ++dj)
        for (int di = -r; di <= r; ++di) {
          const int ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj, ak = dk < 0 ? -dk : dk;
          const int cheb = ai > aj ? (ai > ak ? ai : ak) : (aj > ak ? aj : ak);
          if (cheb != r || g.blocked(v[0] + di, v[1] + dj, v[2] + dk)) continue;
          const int d2 = di * di + dj * dj + dk * dk;
          if (d2 < best) best = d2, bv[0] = v[0] + di, bv[1] = v[1] + dj, bv[2] = v[2] + dk;
        }
    if (best < (1 << 30)) {
      v[0] = bv[0], v[1] = bv[1], v[2] = bv[2];
      return true;
    }
  }
  return false;
}

// steps 1-4: the goal, the start and goal voxels, the last candidate point (G or the moved goal voxel's centre)
struct Ends {
  int sv[3], gv[3];
  V3 gq;
};
CD_HD int path_setup(const PathIn& in, Ends* e) {
  const long long padded = (long long)(in.g.dim[0] + 2) * (in.g.dim[1] + 2) * in.g.dim[2];
  if (in.g.dim[0] < 1 || in.g.dim[1] < 1 || in.g.dim[2] < 1 || padded > 32LL * PLANE_WORDS) return PATH_WORKSPACE;
  const V3 G = intermediate_goal(in.goal, in.origin, in.g.dim, in.res);
  voxel_of(in, in.start, e->sv);
  voxel_of(in, G, e->gv);
  const int g0[3] = {e->gv[0], e->gv[1], e->gv[2]};
  if (!nearest_free(in.g, e->sv) || !nearest_free(in.g, e->gv)) return PATH_NO_FREE_VOXEL;
  const bool moved = g0[0] != e->gv[0] || g0[1] != e->gv[1] || g0[2] != e->gv[2];
  e->gq = moved ? centre(in, e->gv[0], e->gv[1], e->gv[2]) : G;
  return PATH_OK;
}

// "clear" of step 7: raycast (swarm_core.h) from a to b on the local grid, in local voxel units, reports no collision. The
// distance limit is the segment's length plus two voxels: Raycast measures the distance to a voxel's CORNER, which on a segment
// that runs towards negative coordinates can exceed the length by up to sqrt(3) voxels before the last voxels are tested.
CD_HD bool segment_clear(const PathIn& in, const V3& a, const V3& b) {
  V3 s, t;
  for (int ax = 0; ax < 3; ++ax) s[ax] = (a[ax] - in.origin[ax]) / in.res, t[ax] = (b[ax] - in.origin[ax]) / in.res;
  V3 hit = {{-1, -1, -1}};
  return !hdsm_sw::raycast(in.g, s, t, hdsm_sw::norm(hdsm_sw::sub(s, t)) + 2.0, &hit, [](const V3&) {});
}

// step 6, one step: the first neighbour (-x, +x, -y, +y, -z, +z) of `v` inside the grid whose level is `want`; code(i, j, k)
// returns the level (or level mod 3 on the device: neighbouring BFS levels differ by at most one, so L - 1 is identifiable) or
// a value that never equals `want` for an unvisited voxel. False if there is none (cannot happen after a finished search).
template <class Code>
CD_HD bool descend_step(const PathGrid& g, int v[3], int want, Code code) {
  CD_UNROLL
  for (int t = 0; t < 6; ++t) {
    const int s = (t & 1) ? 1 : -1;  // -x, +x, -y, +y, -z, +z
    const int i = v[0] + (t < 2 ? s : 0), j = v[1] + (t >> 1 == 1 ? s : 0), k = v[2] + (t >= 4 ? s : 0);
    if (g.inside(i, j, k) && code(i, j, k) == want) {
      v[0] = i, v[1] = j, v[2] = k;
      return true;
    }
  }
  return false;
}

// no world: the straight segment (step 9)
CD_HD int free_space_path(const PathIn& in, V3* out, int* n_out) {
  out[0] = in.start, out[1] = in.goal;
  *n_out = 2;
  return PATH_OK;
}

// ---- clearance mode (opt-in): the reference's distance-map planner and ShortenDMPPath after the descent -----------------------
// Agent::GetPath (AC:477-567) runs JPS, then the distance-map planner (DMP: jps3d/src/distance_map_planner/, a shortest-path
// search in a tunnel round the prior path, a step costs 1 + cweight * value(voxel), cweight = 1, 6-connected in 3-D:
// graph_search.cpp:40-46), then ShortenDMPPath (path_tools.cpp:250-312). Steps 1-6 above stay and give the PRIOR path (the
// descent's voxel chain P, start and goal voxel included: the stand-in for the JPS raw path); then, instead of step 7:
//   6a cost     for a voxel step 1 calls free, c(v) = the world value if it is 1..99, else 0 (side faces cleared by ClearBoundary
//               and voxels outside the world: 0). Occupied, unknown and below-ground voxels stay blocked as in step 1: the
//               reference's SetUnknown(99) (AC:487) is deliberately NOT taken over, because the prior path already treats
//               unknown as blocked
//   6b tunnel   DMPlanner::setPath (distance_map_planner.cpp:151-226, dense form): rn = ceil(search_rad / res), hn = rn; the
//               mask is every (nx, ny, nz) in [-rn, rn]^3 with NOT hypot(hypot(nx, ny), nz) > rn, literally in double with libm's
//               hypot (built once on the host: DmpMask); T = the free voxels inside the grid at a mask offset from a voxel of P;
//               search_rad < 0: T = every free voxel. rn > DMP_MAX_RN or more than DMP_FIELD voxels in T -> status 4
//   6c field    exact integers on T: D(gv) = c(gv), D(v) = c(v) + 1 + min over the 6-neighbours u in T of D(u); D(sv) is the
//               path's cost (the reference's g(start) = cMap[start], each step + 1 + cMap[next]; symmetric, so searching from
//               the goal is the same). The cost is an int32, which 100 * MAX_DESCENT always fits (the device keeps D mod 255 per voxel and
//               the cost itself as the time of the search, see plan_dmp_block: nothing can overflow)
//   6d descent  from sv, each step to the first neighbour (-x, +x, -y, +y, -z, +z) in T with D(u) == D(v) - 1 - c(v), until gv:
//               a function of D alone, so every form gives the same voxels; more than MAX_DESCENT voxels -> status 4
//   6e raw path S, the centres of the chain's voxels sv .. gv, then G (dropped when step 4 moved the goal voxel) (AC:537-550)
//   7' shorten  ShortenDMPPath statement by statement: the index walk with its erase, IsLineClear with max_dist = |start - end|
//               (path_tools.cpp:148-180), "every visited point <= 0" on the points Raycast hands to `visit`, GetVoxelInt(..) <= 0
//               on both end points (truncation; -1 outside the grid); the grid it sees: 100 for blocked voxels, else c(v).
//               More than PATH_PTS points -> status 3
// One DMP iteration (dmp_n_it: 1 in every shipped configuration); no RemoveZigZagSegments, no stitching.
constexpr int DMP_MAX_RN = 15;                 // tunnel radius in voxels: a row of the mask is one 32-bit word
constexpr int DMP_ROW = 2 * DMP_MAX_RN + 1;
constexpr int DMP_FIELD = 87168;               // voxels of T (device: one byte each in LDS; 66 x 66 x 20 = 87120 fit without a tunnel)

// the tunnel's mask: rows[(nz + rn) * (2 rn + 1) + (ny + rn)] bit (nx + rn); rn < 0: no tunnel
struct DmpMask {
  int rn;
  uint32_t rows[DMP_ROW * DMP_ROW];
};

// what the shortening sees (6a, 7'): blocked voxels 100, else the cost
struct DmpGrid {
  PathGrid g;
  CD_HD bool inside(int i, int j, int k) const { return g.inside(i, j, k); }
  CD_HD int cost(int i, int j, int k) const {  // (i, j, k) inside the grid and free
    if (i == 0 || j == 0 || i == g.dim[0] - 1 || j == g.dim[1] - 1) return 0;
    const int gi = i + g.off[0], gj = j + g.off[1], gk = k + g.off[2];
    if (gi < 0 || gj < 0 || gk < 0 || gi >= g.wdim[0] || gj >= g.wdim[1] || gk >= g.wdim[2]) return 0;
    const int v = g.world[(size_t)gi + (size_t)gj * g.wdim[0] + (size_t)gk * g.wdim[0] * g.wdim[1]];
    return v >= 1 && v <= 99 ? v : 0;
  }
  CD_HD int value(int i, int j, int k) const { return g.occupied(i, j, k) ? 100 : cost(i, j, k); }
  CD_HD int at(const V3& p) const {  // GetVoxelInt(Vector3d): truncation, -1 outside
    const int i = (int)p[0], j = (int)p[1], k = (int)p[2];
    return g.inside(i, j, k) ? value(i, j, k) : -1;
  }
};

CD_HD V3 to_local(const PathIn& in, const V3& p) {
  return {{(p[0] - in.origin[0]) / in.res, (p[1] - in.origin[1]) / in.res, (p[2] - in.origin[2]) / in.res}};
}

// the test of ShortenDMPPath's inner loop for one end point (path_tools.cpp:269-287), s and t in local voxel units
CD_HD bool dmp_segment_ok(const DmpGrid& g, const V3& s, const V3& t) {
  V3 hit = {{-1, -1, -1}};
  bool pot = false;
  const bool collision = hdsm_sw::raycast(g, s, t, hdsm_sw::norm(hdsm_sw::sub(s, t)), &hit, [&](const V3& p) {
    if (g.at(p) > 0) pot = true;
  });
  return g.at(t) <= 0 && !collision && !pot;
}

// step 4 moved the goal voxel (6e: G is dropped)
CD_HD bool goal_moved(const PathIn& in, const Ends& e) {
  int g0[3];
  voxel_of(in, intermediate_goal(in.goal, in.origin, in.g.dim, in.res), g0);
  return g0[0] != e.gv[0] || g0[1] != e.gv[1] || g0[2] != e.gv[2];
}

// The host form of the clearance mode (path_host.cpp). cost = D(sv) and n_raw = voxels of the chain of 6d (-1 / 0 on failure).
bool dmp_build_mask(double search_rad, double res, DmpMask* mask);  // false: rn > DMP_MAX_RN (mask->rn is set all the same)
int plan_dmp_serial(const PathIn& in, const DmpMask& mask, V3* out, int* n_out, int* cost, int* n_raw);

// The host form (path_host.cpp): steps 1-7 with a queue BFS; out[PATH_PTS]. Thread-safe (workspace per thread).
int plan_serial(const PathIn& in, V3* out, int* n_out);

#if defined(__HIPCC__)
// ---- the device form: ONE WORKGROUP (THREADS lanes) per agent, everything in LDS, no scratch ----------------------------------
// Three bit planes of the local grid padded by a guard voxel on each x and y side (x fastest: bit (i + 1) + X ((j + 1) + Y k),
// X = dx + 2, Y = dy + 2): `blocked` (occupied, guard, padding or visited) and the BFS level mod 3 in two planes (lo, hi; 3 = not
// visited). The frontier of level L is read out of the level planes as the voxels of code L mod 3: that also takes the levels
// L - 3, L - 6, ..., whose neighbours are all visited already, so the next level is the same. One level: every thread forms the
// words it owns (six funnel shifts of the frontier, +-1, +-X, +-XY bits — the guard voxels are blocked, so nothing wraps from one
// row into the next — and-not `blocked`) into registers, a barrier, the words are written, a barrier. After the search the
// `blocked` plane holds the descent's voxels.
constexpr int OWN = PLANE_WORDS / THREADS;  // words of a plane per thread
struct PathLds {
  uint32_t blocked[PLANE_WORDS], lo[PLANE_WORDS], hi[PLANE_WORDS];
  V3 out[PATH_PTS];
  int flags, n_out, status, m;
};
static_assert(MAX_DESCENT <= PLANE_WORDS, "the descent is kept in the blocked plane");
static_assert(PLANE_WORDS % THREADS == 0, "words per thread");

__device__ inline uint32_t front_word(const PathLds& s, int W, int idx, uint32_t cl, uint32_t ch) {  // frontier bits of word idx
  return (idx >= 0 && idx < W) ? (~(s.lo[idx] ^ cl) & ~(s.hi[idx] ^ ch)) : 0u;
}
__device__ inline uint32_t shifted_front(const PathLds& s, int W, int w, int sh, uint32_t cl, uint32_t ch) {  // moved by sh bits up
  if (sh >= 0) {
    const int q = sh >> 5, r = sh & 31;
    const uint32_t a = front_word(s, W, w - q, cl, ch);
    return r == 0 ? a : ((a << r) | (front_word(s, W, w - q - 1, cl, ch) >> (32 - r)));
  }
  const int q = (-sh) >> 5, r = (-sh) & 31;
  const uint32_t a = front_word(s, W, w + q, cl, ch);
  return r == 0 ? a : ((a >> r) | (front_word(s, W, w + q + 1, cl, ch) << (32 - r)));
}

// steps 1-6 by the whole workgroup (a world is given): the ends in `e`, the start voxel's level in `L`, the descent's voxels
// (padded bit indices, start voxel first, L + 1 of them) in the blocked plane; the status returned in every thread
__device__ inline int search_block(const PathIn& in, PathLds& lds, int tid, Ends& e, int& L) {
  int st = path_setup(in, &e);  // (every thread: same result, no shared state)
  if (st != PATH_OK) return st;
  const int X = in.g.dim[0] + 2, Y = in.g.dim[1] + 2, Z = in.g.dim[2], XY = X * Y, nbits = XY * Z, W = (nbits + 31) >> 5;
  auto pidx = [&](int i, int j, int k) { return (i + 1) + X * ((j + 1) + Y * k); };
  uint32_t* B = lds.blocked;
  uint32_t* lo = lds.lo;
  uint32_t* hi = lds.hi;
  // init: 64 bits per wavefront step, one voxel per lane (coalesced reads of the world), a ballot makes two words
  const int lane = tid & 63, wave = tid >> 6;
  for (int c = wave; 2 * c < W; c += THREADS / 64) {
    const int b = 64 * c + lane;
    bool blk = true;
    if (b < nbits) {
      const int k = b / XY, r = b - k * XY, jj = r / X, ii = r - jj * X;
      blk = ii == 0 || jj == 0 || ii == X - 1 || jj == Y - 1 || in.g.occupied(ii - 1, jj - 1, k);
    }
    const unsigned long long m = __ballot(blk);
    if (lane < 2 && 2 * c + lane < W) {
      B[2 * c + lane] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
      lo[2 * c + lane] = ~0u, hi[2 * c + lane] = ~0u;
    }
  }
  __syncthreads();
  const int sp = pidx(e.sv[0], e.sv[1], e.sv[2]), gp = pidx(e.gv[0], e.gv[1], e.gv[2]);
  if (tid == 0) {
    const uint32_t bit = 1u << (gp & 31);
    B[gp >> 5] |= bit, lo[gp >> 5] &= ~bit, hi[gp >> 5] &= ~bit;  // level 0
    lds.flags = 0;
  }
  __syncthreads();
  // step 5: level-synchronous BFS; flags bit 0 = the new level is not empty, bit 1 = it holds the start
  L = 0;
  if (sp != gp) {
    for (;;) {
      const uint32_t cl = (L % 3) & 1 ? ~0u : 0u, ch = (L % 3) & 2 ? ~0u : 0u;
      const int code = (L + 1) % 3;
      uint32_t nx[OWN];
      int f = 0;
#pragma unroll
      for (int u = 0; u < OWN; ++u) {
        const int w = tid + u * THREADS;
        uint32_t v = 0u;
        if (w < W) {
          v = shifted_front(lds, W, w, 1, cl, ch) | shifted_front(lds, W, w, -1, cl, ch) | shifted_front(lds, W, w, X, cl, ch) |
              shifted_front(lds, W, w, -X, cl, ch) | shifted_front(lds, W, w, XY, cl, ch) | shifted_front(lds, W, w, -XY, cl, ch);
          v &= ~B[w];
        }
        nx[u] = v;
        if (v) {
          f |= 1;
          if (w == (sp >> 5) && ((v >> (sp & 31)) & 1u)) f |= 2;
        }
      }
      __syncthreads();  // (every frontier word has been read)
#pragma unroll
      for (int u = 0; u < OWN; ++u) {
        const int w = tid + u * THREADS;
        const uint32_t v = nx[u];
        if (v) {
          B[w] |= v;
          lo[w] = (lo[w] & ~v) | ((code & 1) ? v : 0u);
          hi[w] = (hi[w] & ~v) | ((code & 2) ? v : 0u);
        }
      }
      if (f) atomicOr(&lds.flags, f);
      __syncthreads();
      f = lds.flags;
      ++L;
      if (f & 2) break;
      if (!(f & 1)) return PATH_UNREACHABLE;
      __syncthreads();  // (every thread has read the flags)
      if (tid == 0) lds.flags = 0;
    }
  }
  // L = the start voxel's level. Step 6 (one lane): the voxels of the descent into the blocked plane
  if (L + 1 > MAX_DESCENT) return PATH_WORKSPACE;
  int* list = reinterpret_cast<int*>(lds.blocked);
  __syncthreads();  // (the blocked plane is free from here on)
  if (tid == 0) {
    auto code3 = [&](int i, int j, int k) {
      const int p = pidx(i, j, k);
      return (int)((lo[p >> 5] >> (p & 31)) & 1u) | (int)(((hi[p >> 5] >> (p & 31)) & 1u) << 1);
    };
    int v[3] = {e.sv[0], e.sv[1], e.sv[2]};
    int s = PATH_OK;
    list[0] = pidx(v[0], v[1], v[2]);
    for (int lv = L; lv > 0; --lv) {
      if (!descend_step(in.g, v, (lv - 1) % 3, code3)) {
        s = PATH_UNREACHABLE;
        break;
      }
      list[L - lv + 1] = pidx(v[0], v[1], v[2]);
    }
    lds.status = s;
    lds.m = L > 0 ? L : 1;  // (start voxel = goal voxel: the candidates are [S, G])
    lds.out[0] = in.start;
    lds.n_out = 1;
  }
  __syncthreads();
  return lds.status;
}

// steps 1-7 by the whole workgroup; the result in lds.out / lds.n_out, the status returned in every thread
__device__ inline int plan_block(const PathIn& in, PathLds& lds, int tid) {
  if (in.g.world == nullptr) {
    if (tid == 0) lds.status = free_space_path(in, lds.out, &lds.n_out);
    __syncthreads();
    return lds.status;
  }
  Ends e;
  int L;
  int st = search_block(in, lds, tid, e, L);
  if (st != PATH_OK) return st;
  const int X = in.g.dim[0] + 2, Y = in.g.dim[1] + 2, XY = X * Y;
  const int lane = tid & 63, wave = tid >> 6;
  const int* list = reinterpret_cast<const int*>(lds.blocked);
  // step 7 (first wavefront): 64 candidates j tested at once from the top down, the highest clear one taken (ballot)
  if (wave == 0) {
    const int m = lds.m;
    auto q = [&](int t) {
      if (t == 0) return in.start;
      if (t == m) return e.gq;
      const int p = list[t], k = p / XY, r = p - k * XY, jj = r / X, ii = r - jj * X;
      return centre(in, ii - 1, jj - 1, k);
    };
    int a = 0, n = 1;
    while (a < m) {
      int j = a + 1;
      const V3 qa = q(a);
      for (int top = m; top > a + 1; top -= 64) {
        const int cand = top - lane;
        const bool ok = cand > a + 1 && segment_clear(in, qa, q(cand));
        const unsigned long long bal = __ballot(ok);
        if (bal) {
          j = top - (__ffsll((long long)bal) - 1);
          break;
        }
      }
      if (n == PATH_PTS) {
        st = PATH_TOO_LONG;
        break;
      }
      if (lane == 0) lds.out[n] = q(j);
      ++n, a = j;
    }
    if (lane == 0) lds.n_out = n, lds.status = st;
  }
  __syncthreads();
  return lds.status;
}

// ---- the clearance mode on the device: ONE WORKGROUP per agent, everything in LDS, no scratch ---------------------------------
// After search_block the level planes are free: `lo` becomes the bit plane of T (the tunnel's rows OR-ed in by atomics, then
// and-not the occupancy, formed again from the world), `hi` the exclusive prefix of its popcounts, so a voxel of T has a rank and
// the field is COMPACT: one byte per voxel of T. The field is found in the event form: because the weight sits on the target
// voxel, D(v) = (time its first neighbour settles) + 1 + c(v). So a voxel is written once, when first touched, with the code of
// the time it fires (time mod 255, + 1; 0 = not touched), and at time t the voxels whose byte is code(t) touch their untouched
// neighbours. Pending times lie in (t, t + 100], so a 128-bit ring of the times that have an event says which tick is next (empty
// ticks are skipped) and the codes of pending voxels are unambiguous; a SETTLED voxel whose code comes round again fires once
// more, which does nothing, since its neighbours are all touched (the level planes' mod-3 argument). D of two neighbours
// differs by at most 100, so the descent identifies D(v) - 1 - c(v) by its code. The search stops when the start voxel is
// touched: every voxel with a smaller D was touched before. The new chain goes where the prior one was (the blocked plane).
struct alignas(16) DmpLds {
  PathLds p;
  alignas(16) uint8_t field[DMP_FIELD];
  uint32_t ring[4];
  uint32_t wsum[THREADS / 64];
  int cost, n_raw;
};
static_assert(sizeof(DmpLds) <= 160 * 1024, "the clearance mode's LDS");
static_assert(DMP_FIELD % 4 == 0, "the field is cleared and scanned as words");

__device__ inline int plan_dmp_block(const PathIn& in, int rn, const uint32_t* __restrict__ rows, DmpLds& s, int tid) {
  PathLds& lds = s.p;
  if (in.g.world == nullptr) {
    if (tid == 0) lds.status = free_space_path(in, lds.out, &lds.n_out), s.cost = 0, s.n_raw = 0;
    __syncthreads();
    return lds.status;
  }
  if (rn > DMP_MAX_RN) return PATH_WORKSPACE;
  Ends e;
  int L;
  int st = search_block(in, lds, tid, e, L);
  if (st != PATH_OK) return st;
  const int dx = in.g.dim[0], dy = in.g.dim[1];
  const int X = dx + 2, Y = dy + 2, Z = in.g.dim[2], XY = X * Y, nbits = XY * Z, W = (nbits + 31) >> 5;
  const int lane = tid & 63, wave = tid >> 6;
  const DmpGrid dg{in.g};
  uint32_t* T = lds.lo;
  uint32_t* PRE = lds.hi;
  int* list = reinterpret_cast<int*>(lds.blocked);
  auto pidx = [&](int i, int j, int k) { return (i + 1) + X * ((j + 1) + Y * k); };
  // 6b: the tunnel's rows round every voxel of the prior chain, clipped to the grid
  for (int w = tid; w < W; w += THREADS) T[w] = rn < 0 ? ~0u : 0u;
  __syncthreads();
  if (rn >= 0) {
    const int R = 2 * rn + 1, per = R * R, items = (L + 1) * per;
    for (int it = tid; it < items; it += THREADS) {
      const int ci = it / per, r = it - ci * per, nz = r / R - rn, ny = r - (r / R) * R - rn;
      const int p = list[ci], k = p / XY, rr = p - k * XY, jj = rr / X, ii = rr - jj * X;
      const int j2 = jj - 1 + ny, k2 = k + nz, i0 = ii - 1 - rn;  // i0: x of the row's bit 0
      uint32_t m = rows[r];
      if (j2 < 0 || j2 >= dy || k2 < 0 || k2 >= Z) continue;
      if (i0 < 0) m &= ~0u << (-i0);
      if (dx - 1 - i0 < 31) m &= (2u << (dx - 1 - i0)) - 1u;
      if (m == 0u) continue;
      const int tz = __ffs((int)m) - 1;
      m >>= tz;
      const int base = pidx(i0 + tz, j2, k2), w = base >> 5, sh = base & 31;
      atomicOr(&T[w], m << sh);
      if (sh != 0 && (m >> (32 - sh)) != 0u) atomicOr(&T[w + 1], m >> (32 - sh));
    }
  }
  __syncthreads();
  for (int c = wave; 2 * c < W; c += THREADS / 64) {  // and-not the occupancy (as search_block's init forms it)
    const int b = 64 * c + lane;
    bool blk = true;
    if (b < nbits) {
      const int k = b / XY, r = b - k * XY, jj = r / X, ii = r - jj * X;
      blk = ii == 0 || jj == 0 || ii == X - 1 || jj == Y - 1 || in.g.occupied(ii - 1, jj - 1, k);
    }
    const unsigned long long m = __ballot(blk);
    if (lane < 2 && 2 * c + lane < W) T[2 * c + lane] &= ~(lane ? (uint32_t)(m >> 32) : (uint32_t)m);
  }
  __syncthreads();
  // ranks: thread t owns the words [OWN t, OWN t + OWN)
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < OWN; ++u) {
    const int w = OWN * tid + u;
    if (w < W) cnt += __popc(T[w]);
  }
  int inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d);
    if (lane >= d) inc += v;
  }
  if (lane == 63) s.wsum[wave] = (uint32_t)inc;
  __syncthreads();
  int run = inc - cnt, NT = 0;
  for (int q = 0; q < THREADS / 64; ++q) {
    const int v = (int)s.wsum[q];
    if (q < wave) run += v;
    NT += v;
  }
#pragma unroll
  for (int u = 0; u < OWN; ++u) {
    const int w = OWN * tid + u;
    if (w < W) PRE[w] = (uint32_t)run, run += __popc(T[w]);
  }
  if (NT > DMP_FIELD) return PATH_WORKSPACE;
  uint32_t* F4 = reinterpret_cast<uint32_t*>(s.field);
  const int NT4 = (NT + 3) >> 2;
  for (int q = tid; q < NT4; q += THREADS) F4[q] = 0u;
  if (tid < 4) s.ring[tid] = 0u;
  __syncthreads();
  auto in_t = [&](int p) { return p >= 0 && p < nbits && ((T[p >> 5] >> (p & 31)) & 1u) != 0u; };
  auto rank = [&](int p) { return (int)PRE[p >> 5] + __popc(T[p >> 5] & ((1u << (p & 31)) - 1u)); };
  auto cost_at = [&](int p) {
    const int k = p / XY, r = p - k * XY, jj = r / X, ii = r - jj * X;
    return dg.cost(ii - 1, jj - 1, k);
  };
  auto code = [](int t) { return (uint32_t)(t % 255 + 1); };
  const int nb[6] = {-1, 1, -X, X, -XY, XY};
  const int sp = pidx(e.sv[0], e.sv[1], e.sv[2]), gp = pidx(e.gv[0], e.gv[1], e.gv[2]);
  // 6c: the field, until the start voxel is touched
  int cost = cost_at(gp);
  if (sp != gp) {
    int t = cost;
    if (tid == 0) s.field[rank(gp)] = (uint8_t)code(t);
    const int rs = rank(sp);
    __syncthreads();
    for (;;) {
      const uint32_t cd = code(t), pat = cd * 0x01010101u;
      for (int q = tid; q < NT4; q += THREADS) {
        const uint32_t x = F4[q] ^ pat;
        if (((x - 0x01010101u) & ~x & 0x80808080u) == 0u) continue;  // no byte of the word is code(t)
        for (int b = 0; b < 4; ++b) {
          const int idx = 4 * q + b;
          if (((x >> (8 * b)) & 0xffu) != 0u || idx >= NT) continue;
          int wl = 0, wh = W - 1;  // the voxel of rank idx: the last word whose prefix is <= idx, its (idx - prefix)-th bit
          while (wl < wh) {
            const int mid = (wl + wh + 1) >> 1;
            if ((int)PRE[mid] <= idx) wl = mid;
            else wh = mid - 1;
          }
          uint32_t m = T[wl];
          for (int kk = idx - (int)PRE[wl]; kk > 0; --kk) m &= m - 1u;
          const int p = 32 * wl + __ffs((int)m) - 1;
#pragma unroll
          for (int o = 0; o < 6; ++o) {
            const int p2 = p + nb[o];
            if (!in_t(p2)) continue;
            const int r2 = rank(p2);
            if (s.field[r2] != 0) continue;
            const int ft = t + 1 + cost_at(p2);
            s.field[r2] = (uint8_t)code(ft);
            atomicOr(&s.ring[(ft >> 5) & 3], 1u << (ft & 31));
          }
        }
      }
      __syncthreads();
      if (s.field[rs] != 0) {  // touched at time t
        cost = t + 1 + cost_at(sp);
        break;
      }
      const unsigned long long r0 = s.ring[0] | ((unsigned long long)s.ring[1] << 32), r1 = s.ring[2] | ((unsigned long long)s.ring[3] << 32);
      int sh = (t + 1) & 127;  // the first set bit at or after time t + 1
      unsigned long long a = r0, b = r1;
      if (sh >= 64) a = r1, b = r0, sh -= 64;
      if (sh != 0) {
        const unsigned long long a2 = (a >> sh) | (b << (64 - sh)), b2 = (b >> sh) | (a << (64 - sh));
        a = a2, b = b2;
      }
      if (a == 0ull && b == 0ull) return PATH_UNREACHABLE;  // (cannot happen: the prior chain lies in T)
      t = t + 1 + (a != 0ull ? __ffsll((long long)a) - 1 : 64 + __ffsll((long long)b) - 1);
      __syncthreads();  // (every thread has read the field and the ring)
      if (tid == 0) atomicAnd(&s.ring[(t >> 5) & 3], ~(1u << (t & 31)));
    }
  }
  __syncthreads();  // (the prior chain and the ring are not read any more)
  // 6d (one lane): the chain into the blocked plane
  if (tid == 0) {
    int v = sp, dv = cost, n = 1, stt = PATH_OK;
    list[0] = sp;
    while (v != gp) {
      const int want = dv - 1 - cost_at(v);
      int nxt = -1;
      if (want >= 0) {
        const uint32_t cd = code(want);
#pragma unroll
        for (int o = 0; o < 6; ++o) {
          const int p2 = v + nb[o];
          if (nxt < 0 && in_t(p2) && s.field[rank(p2)] == cd) nxt = p2;
        }
      }
      if (nxt < 0) {
        stt = PATH_UNREACHABLE;
        break;
      }
      if (n == MAX_DESCENT) {
        stt = PATH_WORKSPACE;
        break;
      }
      list[n++] = nxt, v = nxt, dv = want;
    }
    lds.status = stt, s.n_raw = n, s.cost = cost;
  }
  __syncthreads();
  st = lds.status;
  if (st != PATH_OK) return st;
  // 6e, 7' (first wavefront): from q_a the candidates a + 1, a + 2, ... 64 at a time, up to the first that fails (ballot)
  if (wave == 0) {
    const int n_raw = s.n_raw, npts = 1 + n_raw + (goal_moved(in, e) ? 0 : 1);
    auto q = [&](int t) {
      if (t == 0) return in.start;
      if (t > n_raw) return e.gq;
      const int p = list[t - 1], k = p / XY, r = p - k * XY, jj = r / X, ii = r - jj * X;
      return centre(in, ii - 1, jj - 1, k);
    };
    int a = 0, n = 0;
    for (;;) {
      if (n == PATH_PTS) {
        st = PATH_TOO_LONG;
        break;
      }
      const V3 qa = q(a);
      if (lane == 0) lds.out[n] = qa;
      ++n;
      if (a >= npts - 1) break;
      int next = a + 1;
      const V3 la = to_local(in, qa);
      if (dg.at(la) <= 0) {
        int i_end = npts - 1;
        for (int base = a + 1; base < npts; base += 64) {
          const int cand = base + lane;
          const bool bad = cand < npts && !dmp_segment_ok(dg, la, to_local(in, q(cand)));
          const unsigned long long bal = __ballot(bad);
          if (bal) {
            i_end = base + (__ffsll((long long)bal) - 1) - 1;
            break;
          }
        }
        if (i_end > a) next = i_end;
      }
      a = next;
    }
    if (lane == 0) lds.n_out = n, lds.status = st;
  }
  __syncthreads();
  return lds.status;
}
#endif

}  // namespace hdsm_path
