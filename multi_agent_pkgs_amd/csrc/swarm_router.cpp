// swarm_router.cpp — a minimal router on the world grid of the host mirror (see hdsm_swarm_route in include/hdsm_swarm.h). Pure host C++.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <queue>
#include <thread>
#include <vector>

#include "swarm_host.h"

using namespace hdsm_mirror;

namespace {

using hdsm_sw::axpy;

struct Router {
  // what the router sees of the mirror: the world grid and the planner's local grid over it
  struct Grid {
    const int8_t* world;
    int dim[3];
    double origin[3];
    double voxel_size, grid_z_min, grid_range_z;
  };
  const Grid gr;
  std::vector<uint8_t> cls;  // 0 free, 1 within two voxels of an obstacle, 2 occupied (or below the ground)
  int nx, ny, nz;
  explicit Router(const Grid& g) : gr(g), nx(g.dim[0]), ny(g.dim[1]), nz(g.dim[2]) {
    const size_t tot = (size_t)nx * ny * nz;
    cls.assign(tot, 0);
    const double vs = gr.voxel_size;
    const int k_ground = (int)std::ceil((gr.grid_z_min - gr.origin[2]) / vs - 1e-9);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          const int8_t v = gr.world[idx(i, j, k)];
          if (v >= 100 || v < 0 || k < k_ground) cls[idx(i, j, k)] = 2;
        }
    // "near" band: separable box dilation of the occupied set by two voxels
    std::vector<uint8_t> a(tot), b(tot);
    for (size_t t = 0; t < tot; ++t) a[t] = cls[t] == 2;
    auto pass = [&](const std::vector<uint8_t>& in, std::vector<uint8_t>& out, int ax) {
      const int n[3] = {nx, ny, nz};
      const size_t st[3] = {1, (size_t)nx, (size_t)nx * ny};
      for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
          for (int i = 0; i < nx; ++i) {
            const int c[3] = {i, j, k};
            uint8_t v = 0;
            for (int d = -2; d <= 2 && !v; ++d) {
              const int q = c[ax] + d;
              if (q >= 0 && q < n[ax]) v = in[idx(i, j, k) + (size_t)((long)d * (long)st[ax])];
            }
            out[idx(i, j, k)] = v;
          }
    };
    pass(a, b, 0), pass(b, a, 1), pass(a, b, 2);
    for (size_t t = 0; t < tot; ++t)
      if (b[t] && cls[t] == 0) cls[t] = 1;
  }
  size_t idx(int i, int j, int k) const { return (size_t)i + (size_t)j * nx + (size_t)k * nx * ny; }
  bool in(int i, int j, int k) const { return i >= 0 && j >= 0 && k >= 0 && i < nx && j < ny && k < nz; }
  bool blocked(int i, int j, int k) const { return !in(i, j, k) || cls[idx(i, j, k)] == 2; }
  void voxel_of(const V3& p, int v[3]) const {
    for (int ax = 0; ax < 3; ++ax) v[ax] = (int)std::floor((p[ax] - gr.origin[ax]) / gr.voxel_size);
  }
  V3 centre(int i, int j, int k) const {
    const double vs = gr.voxel_size;
    return {gr.origin[0] + (i + 0.5) * vs, gr.origin[1] + (j + 0.5) * vs, gr.origin[2] + (k + 0.5) * vs};
  }
  // every voxel touched by the segment (sampled at a quarter voxel) is free — with `strict`, also outside the band next to
  // obstacles; points outside the world count as blocked
  bool line_clear(const V3& a, const V3& b, bool strict = false) const {
    const double len = norm(sub(b, a)), step = gr.voxel_size / 4;
    const int n = (int)std::ceil(len / step);
    for (int t = 0; t <= n; ++t) {
      const V3 p = axpy(a, n ? (double)t / n : 0.0, sub(b, a));
      int v[3];
      voxel_of(p, v);
      if (blocked(v[0], v[1], v[2])) return false;
      if (strict && cls[idx(v[0], v[1], v[2])] != 0) return false;
    }
    return true;
  }
  // nearest free voxel to v (breadth-first over a small cube), false if none within 6 voxels
  bool nearest_free(int v[3]) const {
    if (!blocked(v[0], v[1], v[2])) return true;
    for (int r = 1; r <= 6; ++r) {
      double best = 1e300;
      int bv[3] = {0, 0, 0};
      for (int dk = -r; dk <= r; ++dk)
        for (int dj = -r; dj <= r; ++dj)
          for (int di = -r; di <= r; ++di) {
            if (std::max(std::abs(di), std::max(std::abs(dj), std::abs(dk))) != r) continue;
            if (blocked(v[0] + di, v[1] + dj, v[2] + dk)) continue;
            const double d2 = di * di + dj * dj + dk * dk;
            if (d2 < best) best = d2, bv[0] = v[0] + di, bv[1] = v[1] + dj, bv[2] = v[2] + dk;
          }
      if (best < 1e300) {
        v[0] = bv[0], v[1] = bv[1], v[2] = bv[2];
        return true;
      }
    }
    return false;
  }
  // weighted A* (26-connected, Euclidean heuristic x 2: greedy enough to run straight through a forest and to flood only
  // the face of a wall until it finds a gap; cells of the near band cost 2x), searched inside a box around start and goal
  // (dense arrays, one workspace per thread), then greedy shortening. The whole world is searched if the box has no route.
  struct Work {
    std::vector<float> g;
    std::vector<int32_t> parent;
    std::vector<uint8_t> state;
  };
  bool route(const V3& start, const V3& goal, std::vector<V3>* out, Work& wk) const {
    int s[3], g[3];
    voxel_of(start, s), voxel_of(goal, g);
    if (!in(s[0], s[1], s[2]) || !in(g[0], g[1], g[2])) return false;
    if (!nearest_free(s) || !nearest_free(g)) return false;
    // the planner only ever sees a local grid of grid_range[2] metres of height around the agent: the route stays within
    // half of that above and below the start / goal altitudes (it does not climb over a forest)
    const int band = (int)std::floor(0.5 * gr.grid_range_z / gr.voxel_size);
    const int n[3] = {nx, ny, nz};
    std::vector<int32_t> chain;
    int lo[3], hi[3], ext[3];
    bool found = false;
    for (int attempt = 0; attempt < 2 && !found; ++attempt) {
      const int margin[3] = {attempt ? nx : 12, attempt ? ny : 40, band};
      size_t cells = 1;
      for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = std::max(0, std::min(s[ax], g[ax]) - margin[ax]);
        hi[ax] = std::min(n[ax] - 1, std::max(s[ax], g[ax]) + margin[ax]);
        ext[ax] = hi[ax] - lo[ax] + 1;
        cells *= (size_t)ext[ax];
      }
      if (cells > (size_t)400000000) return false;
      wk.g.assign(cells, 0.0f), wk.parent.assign(cells, -1), wk.state.assign(cells, 0);
      auto lid = [&](int i, int j, int k) { return (int32_t)((i - lo[0]) + ext[0] * ((j - lo[1]) + ext[1] * (k - lo[2]))); };
      auto h = [&](int i, int j, int k) {
        const double a = i - g[0], b = j - g[1], c = k - g[2];
        return 2.0 * std::sqrt(a * a + b * b + c * c);
      };
      struct Node {
        float f;
        int32_t id;
        bool operator<(const Node& o) const { return f > o.f; }
      };
      std::priority_queue<Node> open;
      const int32_t sid = lid(s[0], s[1], s[2]), gid = lid(g[0], g[1], g[2]);
      wk.state[sid] = 1, wk.parent[sid] = sid;
      open.push({(float)h(s[0], s[1], s[2]), sid});
      while (!open.empty()) {
        const Node cur = open.top();
        open.pop();
        if (wk.state[cur.id] == 2) continue;
        wk.state[cur.id] = 2;
        if (cur.id == gid) {
          found = true;
          break;
        }
        const int ci = lo[0] + cur.id % ext[0], cj = lo[1] + (cur.id / ext[0]) % ext[1], ck = lo[2] + cur.id / (ext[0] * ext[1]);
        const float gc = wk.g[cur.id];
        for (int dk = -1; dk <= 1; ++dk)
          for (int dj = -1; dj <= 1; ++dj)
            for (int di = -1; di <= 1; ++di) {
              if (!di && !dj && !dk) continue;
              const int ni = ci + di, nj = cj + dj, nk = ck + dk;
              if (ni < lo[0] || ni > hi[0] || nj < lo[1] || nj > hi[1] || nk < lo[2] || nk > hi[2]) continue;
              if (blocked(ni, nj, nk)) continue;
              // no squeezing diagonally between two blocked voxels
              if (di && dj && (blocked(ci + di, cj, ck) || blocked(ci, cj + dj, ck))) continue;
              if (di && dk && (blocked(ci + di, cj, ck) || blocked(ci, cj, ck + dk))) continue;
              if (dj && dk && (blocked(ci, cj + dj, ck) || blocked(ci, cj, ck + dk))) continue;
              const int32_t nid = lid(ni, nj, nk);
              if (wk.state[nid] == 2) continue;
              const float w = std::sqrt((float)(di * di + dj * dj + dk * dk)) * (cls[idx(ni, nj, nk)] == 1 ? 2.0f : 1.0f);
              const float ng = gc + w;
              if (wk.state[nid] == 0 || ng < wk.g[nid]) {
                wk.state[nid] = 1, wk.g[nid] = ng, wk.parent[nid] = cur.id;
                open.push({ng + (float)h(ni, nj, nk), nid});
              }
            }
      }
      if (found) {
        for (int32_t id = gid;; id = wk.parent[id]) {
          chain.push_back(id);
          if (id == sid) break;
        }
      }
    }
    if (!found) return false;
    std::vector<V3> raw;
    for (auto it = chain.rbegin(); it != chain.rend(); ++it)
      raw.push_back(centre(lo[0] + *it % ext[0], lo[1] + (*it / ext[0]) % ext[1], lo[2] + *it / (ext[0] * ext[1])));
    // the true end points replace the voxel centres when they can be reached in a straight line
    if (line_clear(start, raw.front())) raw.insert(raw.begin(), start);
    if (line_clear(raw.back(), goal)) raw.push_back(goal);
    out->clear();
    out->push_back(raw.front());
    size_t i = 0;
    while (i + 1 < raw.size()) {
      size_t j = raw.size() - 1;
      // shortcuts keep the clearance the search paid for: they may not enter the band next to obstacles (where the raw path
      // itself runs through that band — a narrow passage — its cells are kept one by one)
      while (j > i + 1 && !line_clear(raw[i], raw[j], true)) --j;
      if (j == i + 1) {  // inside the band: plain line of sight, over a short stretch only
        j = std::min(raw.size() - 1, i + 20);
        while (j > i + 1 && !line_clear(raw[i], raw[j])) --j;
      }
      out->push_back(raw[j]);
      i = j;
    }
    return out->size() >= 2;
  }
};

}  // namespace

extern "C" int hdsm_swarm_route(void* swarm, int32_t* n_failed) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !sw->world.has) return HDSM_ERR_BAD_ARG;
  const World& w = sw->world;
  const Router router(Router::Grid{w.grid.data(), {w.dim[0], w.dim[1], w.dim[2]}, {w.origin[0], w.origin[1], w.origin[2]},
                                   sw->cfg.voxel_size, sw->cfg.grid_z_min, sw->cfg.grid_range[2]});
  std::atomic<int> failed{0}, next{0};
  auto worker = [&]() {
    Router::Work wk;
    for (int k = next.fetch_add(1); k < sw->n_local; k = next.fetch_add(1)) {
      AgentS& ag = sw->agents[k];
      std::vector<V3> path;
      bool ok = router.route(ag.start, ag.goal, &path, wk);
      if (ok) {
        // the reference sampling starts ON the path and corridor seeds are taken along it: the first point is the start
        if (norm(sub(path.front(), ag.start)) > 0) path.insert(path.begin(), ag.start);
        if (norm(sub(path.back(), ag.goal)) > 0) path.push_back(ag.goal);
        ok = (int)path.size() <= hdsm_sw::PATH_PTS;
      }
      if (ok) {
        ag.n_path = (int)path.size();
        for (int i = 0; i < ag.n_path; ++i) ag.path[i] = path[i];
      } else {
        ag.n_path = 2, ag.path[0] = ag.start, ag.path[1] = ag.goal;
        failed.fetch_add(1);
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 64 ? 64 : nt);
  if ((int)nt > sw->n_local) nt = (unsigned)(sw->n_local > 0 ? sw->n_local : 1);
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
  if (n_failed) *n_failed = failed.load();
  return HDSM_OK;
}
