// path_core.h — the path step of Agent::UpdatePath (AC:261-454) for one agent, as plain functions that compile for the host form
// (path_host.cpp: hdsm_local_path_host, the host mirror's hdsm_swarm_replan_paths / path period) AND for the device (k_path in
// swarm_kernels.hip, k_path_batch in path_kernels.hip): one source for the grid, the goal, the start, the descent and the
// shortening, so the two give the same points bit for bit. AC = multi_agent_planner/src/agent_class.cpp of the reference.
//
// NOT the reference's planner: UpdatePath runs JPS3D + a distance-map planner (DMP) and ShortenDMPPath. This is a stated
// stand-in, like the host router of hdsm_swarm_route — a breadth-first search on the same local grid with a greedy
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

// steps 1-7 by the whole workgroup; the result in lds.out / lds.n_out, the status returned in every thread
__device__ inline int plan_block(const PathIn& in, PathLds& lds, int tid) {
  if (in.g.world == nullptr) {
    if (tid == 0) lds.status = free_space_path(in, lds.out, &lds.n_out);
    __syncthreads();
    return lds.status;
  }
  Ends e;
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
  int L = 0;
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
  st = lds.status;
  if (st != PATH_OK) return st;
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
#endif

}  // namespace hdsm_path
