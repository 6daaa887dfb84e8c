// swarm_kernels.hip — the device-resident closed loop: the planner state of a shard of agents (hdsm_sw::AgentS) lives in HBM and
// one replan round is a chain of launches on ONE stream with no host round trip:
//   k_corridor   GenerateSafeCorridor (AC:1236-1447; row f2: voxel decomposition on a window of the world grid) + the polyline
//                of this round's reference (AC:1459-1496) + the solver inputs that do not depend on the reference (id, state,
//                corridor rows in the layouts of hdsm.h)                                          one wavefront per agent
//   k_reference  GenerateReferenceTrajectory's neighbour speed term + SamplePath (row f1)       hdsm_reference_device
//   k_replan     planes + MIQP (the hot path)                                                   hdsm_replan_device
//   k_commit     the new reference into the agent state, read-back, shift fallback, increment check, state advance, published
//                record                                                                          one wavefront per agent
//   k_track      (only with a tracking model, hdsm_dswarm_set_tracking) the state flown in place of traj_curr[step_plan] and the record
//                of the difference (track_kernels.hip); also launched between rounds by hdsm_dswarm_set_states*   one lane per flown agent
//   k_script     (only with scripted agents, hdsm_dswarm_set_script) the records of the shard's scripted tail, over the slots
//                k_commit has just padded (script_kernels.hip)                                   one wavefront per scripted agent
//   exchange     ONE RCCL all-gather (hdsm_exchange_device), nothing on a single rank (k_commit publishes straight into the plans
//                buffer), or — the ranks of one process, hdsm_dswarm_round_ranks — ONE k_gather_local per rank (exchange_kernels.hip)
// The per-agent functions are the SAME source as the host mirror (swarm_core.h), which is how the two loops are compared in
// tests/test_gpu_configs.py. AC = multi_agent_planner/src/agent_class.cpp of the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hdsm.h"
#include "../../include/hdsm_swarm.h"
#include "audit_device.h"
#include "device_mem.h"
#include "hdsm_internal.h"
#include "link_core.h"
#include "path_core.h"
#include "script_device.h"
#include "swarm_core.h"
#include "track_device.h"

#ifdef CD_PROFILE
// development builds only: the phase counters of the corridor kernel's decompositions (read and cleared); [12] cycles of the whole
// corridor step, [13] of its decompositions, [14] agent-rounds, [15] decompositions. (The polyhedron cache's counters are NOT in here:
// hdsm_dswarm_cache_stats, every build.)
extern "C" int hdsm_swarm_corridor_profile(unsigned long long out[16]) {
  if (hipDeviceSynchronize() != hipSuccess) return HDSM_ERR_DEVICE;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hdsm_cd::g_cd_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return HDSM_ERR_DEVICE;
  unsigned long long zero[16] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(hdsm_cd::g_cd_prof), zero, sizeof zero) != hipSuccess) return HDSM_ERR_DEVICE;
  return HDSM_OK;
}
#endif

namespace {

using hdsm_sw::AgentS;
using hdsm_sw::Cfg;
using hdsm_sw::V3;

thread_local std::string g_err;
int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(HDSM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int PTS = hdsm_sw::PATH_PTS + 1;  // points of a reference polyline handed to k_reference
// scratch of one agent's voxel decompositions, in LDS (dynamic shared memory of k_corridor): the workspace, the overlay bits and
// the 2-bit cache of the world under the overlay. The decomposition is one lane's chain of small dependent accesses — in global
// memory every one of them was a round trip (33 ms per round for 256 agents in the pillar forest).
constexpr size_t SLAB = hdsm_cd::WAVE_LDS_MAX;  // (the launch asks for what its n_it needs: wave_lds_bytes)
// k_corridor also has static __shared__ state (the walk's rows and flags, < 4 KB); together they must stay inside the 64 KB a
// kernel may use without hipFuncAttributeMaxDynamicSharedMemorySize — a growth of Work / the overlay fails HERE, not at launch
static_assert(SLAB + 4096 <= 64 * 1024, "k_corridor: dynamic + static LDS exceed the default 64 KB limit");

// The polyhedra an agent's last decompositions produced. The corridor keeps only the polyhedra the last plan used, so the ones
// further down the path are dropped and asked for again round after round with the same seed voxel — more than half of all
// decompositions of a forest flight. What a decomposition yields depends on the (constant) world and configuration, on the seed,
// and on the local grid only where the growth meets the grid's border or the ground plane moves; so an entry holds the
// polyhedron as INTEGERS relative to the seed (hdsm_cd::PolyStruct) with the seed's world voxel, the grid's offset in the world,
// the ground plane's world level and whether everything a decomposition can look at (the seed +- wave_map_radius) lay inside the
// grid's interior in x and y. A request for the same world voxel from a grid at the same height with that property too (or from
// the same grid) gets its rows
// formed from the entry — with the arithmetic a decomposition in ITS grid would use, origin included (rows_from_structure), so the
// host mirror, which grows the polyhedron again, gets the same bits.
constexpr int CACHE_POLYS = 6;
constexpr int32_t kCacheHole = INT32_MIN;  // seed_w[.][0] of an entry a map update dropped (k_cache_invalidate): no request has it
struct PolyCache {
  hdsm_cd::PolyStruct ps[CACHE_POLYS];
  int32_t seed_w[CACHE_POLYS][3], off[CACHE_POLYS][3], ground_w[CACHE_POLYS], interior[CACHE_POLYS];
  int32_t n, next;
  // what the cache did for this agent (hdsm_dswarm_cache_stats; written by lane 0 of the agent's own wavefront): polyhedra asked
  // for, found with the same grid, found through the interior rule (another grid at the same height)
  int32_t asked, hits_same_grid, hits_interior, pad_;
};

// GenerateSafeCorridor (AC:1236-1447), ONE WAVEFRONT PER AGENT. The walk along the path (steps of voxel / 10: hundreds of
// them per round) tests every sample against every row of the kept polyhedra; with one thread per agent each test was a chain of
// global loads (1.3 ms per round for 1024 agents). Here the rows live in the registers of the 64 lanes (two rows per lane,
// P * RS <= 128), a sample is tested against all of them at once and `inside` is a ballot; the walk state is computed redundantly
// by every lane (wave-uniform), so the arithmetic — and the result — is exactly that of hdsm_sw::corridor_step. New polyhedra:
// the closed form in free space (lane 0), the voxel decomposition on a window of the world grid by the whole wavefront
// (corridor_wave.h: the world under the overlay classified into bit maps in LDS, layers grown as bit planes).

// min over the 64 lanes of a double, in every lane: four DPP row rotations + four v_readlane (six __shfl_xor stages are twelve
// ds_bpermute round trips)
__device__ __forceinline__ double wave_min_f64(double v) {
  auto rot = [](double x, auto ctrl) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), decltype(ctrl)::value, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), decltype(ctrl)::value, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
  };
  v = fmin(v, rot(v, std::integral_constant<int, 0x121>{}));  // row_ror:1
  v = fmin(v, rot(v, std::integral_constant<int, 0x122>{}));  // row_ror:2
  v = fmin(v, rot(v, std::integral_constant<int, 0x124>{}));  // row_ror:4
  v = fmin(v, rot(v, std::integral_constant<int, 0x128>{}));  // row_ror:8
  auto lane_of = [](double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
  };
  return fmin(fmin(lane_of(v, 0), lane_of(v, 16)), fmin(lane_of(v, 32), lane_of(v, 48)));
}

// (inlined into the kernel: only there does the compiler know that the workspace is LDS — behind a call every access of the
// decomposition was a flat load)
__device__ __forceinline__ void corridor_step_wave(const Cfg& c, AgentS& ag, const hdsm_cd::WaveLds& lds, V3* path, int lane, PolyCache* pc) {
  using namespace hdsm_sw;
  const int P = c.P, N = c.N, RS = c.RS;
  __shared__ int sh_npath;
  // keep-last / keep-used (AC:1253-1282), by the whole wavefront: lane j tests point j of the current plan against the last
  // polyhedron (the verdict is a ballot — the serial loop's early exit does not change it) and a polyhedron that moves to another
  // slot is copied by all lanes (1 KB: one lane copying it was a chain of a hundred global accesses per round)
  static_assert(sizeof(Poly) % 8 == 0, "copied as 8-byte words");
  auto copy_poly = [&](Poly* dst, const Poly* src) {
    const unsigned long long* sw = reinterpret_cast<const unsigned long long*>(src);
    unsigned long long* dw = reinterpret_cast<unsigned long long*>(dst);
    for (int e = lane; e < (int)(sizeof(Poly) / 8); e += 64) dw[e] = sw[e];
  };
  int n_poly = 0;
  {
    const int np0 = ag.n_poly;
    bool kept_last = false;
    if (np0 > 0) {
      bool ok = true;
      if (ag.has_traj && lane <= N) ok = inside(ag.polys[np0 - 1], V3{{ag.traj_curr[lane][0], ag.traj_curr[lane][1], ag.traj_curr[lane][2]}});
      if (__ballot(!ok) == 0ull) {
        if (np0 - 1 != 0) copy_poly(&ag.polys[0], &ag.polys[np0 - 1]);
        n_poly = 1, kept_last = true;
      }
    }
    if (np0 > 0 && !kept_last)
      for (int i = 0; i < P && i < np0; ++i)
        if (ag.poly_used[i]) {
          if (n_poly != i) copy_poly(&ag.polys[n_poly], &ag.polys[i]);
          ++n_poly;
        }
  }
  if (lane == 0) {  // the path ahead (AC:1286-1290): a handful of operations
    ag.corridor_rc = 0;
    const V3 path_head = ag.n_ref == 0 ? ag.path[0] : V3{{ag.traj_ref[0][0], ag.traj_ref[0][1], ag.traj_ref[0][2]}};
    path[0] = {{ag.state_curr[0], ag.state_curr[1], ag.state_curr[2]}};
    sh_npath = 1 + path_ahead(ag, path_head, path + 1);
  }
  __syncthreads();
  const int n_path = sh_npath;
  const double vs = c.voxel_size;
  V3 origin;
  for (int ax = 0; ax < 3; ++ax) origin[ax] = floor((ag.state_curr[ax] - c.grid_range[ax] / 2) / vs) * vs;
  // rows lane and lane + 64 of the flattened [P][RS] table
  double ra[2][4];
  bool rv[2];
  int pj[2];  // the polyhedron the row belongs to (-1: no row)
  auto load_rows = [&]() {
    for (int h = 0; h < 2; ++h) {
      const int lin = lane + 64 * h, j = lin / RS, r = lin % RS;
      rv[h] = j < n_poly && r < ag.polys[j].rows;
      pj[h] = rv[h] ? j : -1;
      for (int q = 0; q < 3; ++q) ra[h][q] = rv[h] ? ag.polys[j].A[r][q] : 0.0;
      ra[h][3] = rv[h] ? ag.polys[j].b[r] : 0.0;
    }
  };
  load_rows();
  int path_idx = 1;
  V3 curr = path[0];
  V3 next = path[1];
  const double samp = vs / 10;  // AC:1316
  // (the shortcut below is pure bookkeeping — it never changes a sample — so it is not tried again where it has just found nothing
  // to skip: same polyhedron, same path segment, closer to the exit than its margin. Computing the exit distance for each of the
  // last samples before an exit was most of this kernel's time in free space.)
  int hold_j = -1, hold_seg = -1;
  while (n_poly < P) {
    const V3 diff = sub(next, curr);
    const double dist_next = norm(diff);
    if (dist_next > samp) {
      curr = step_along(curr, samp, diff, dist_next);
    } else {
      curr = next;
      if (++path_idx == n_path) break;
      next = path[path_idx];
    }
    // inside at least one kept polyhedron? (LinearConstraint::inside: no row with A x - b > 0)
    bool bad[2];
    for (int h = 0; h < 2; ++h) bad[h] = rv[h] && (((ra[h][0] * curr[0] + ra[h][1] * curr[1]) + ra[h][2] * curr[2]) - ra[h][3] > 0);
    int j_in = -1;
    for (int j = 0; j < n_poly; ++j)  // (one ballot per kept polyhedron: the first one without a violated row)
      if (__ballot((bad[0] && pj[0] == j) || (bad[1] && pj[1] == j)) == 0ull) {
        j_in = j;
        break;
      }
    if (j_in >= 0) {
      // The sample lies in polyhedron j_in. While the walk keeps its direction, every sample closer than the exit distance of the
      // ray from that polyhedron is inside it too and the reference loop would just `continue`: those samples are generated
      // (same statements, same rounding) without being tested. The exit distance is a min over the rows held by the lanes; three
      // samples of margin cover the rounding of the accumulated positions.
      if (c.fast_walk && dist_next > samp && !(j_in == hold_j && path_idx == hold_seg)) {
        double t_exit = DBL_MAX;
        for (int h = 0; h < 2; ++h)
          if (pj[h] == j_in) {
            const double rate = ((ra[h][0] * diff[0] + ra[h][1] * diff[1]) + ra[h][2] * diff[2]) / dist_next;
            const double slack = ra[h][3] - ((ra[h][0] * curr[0] + ra[h][1] * curr[1]) + ra[h][2] * curr[2]);
            // every skipped sample keeps a slack >= kWalkTol in every row, far above the rounding of A x - b: a path
            // that slides along a face (slack ~ 0, rate ~ 0) is left to the regular loop, whose outcome there depends
            // on the last bit exactly as the reference's does
            if (!(slack > kWalkTol)) t_exit = 0;
            else if (rate > 0) t_exit = fmin(t_exit, (slack - kWalkTol) / rate);
          }
        t_exit = wave_min_f64(t_exit);
        const double cap = t_exit / samp - 3.0;
        int n_safe = cap > 1e6 ? 1000000 : (cap > 0 ? (int)cap : 0);
        hold_j = n_safe == 0 ? j_in : -1, hold_seg = path_idx;
        if (!c.has_world) {
          // free space: the skipped samples are not even generated one by one (walk_jump). Only where the polyhedra are the
          // large boxes of an empty grid: next to obstacles a routed path slides along faces, the outcome of the first
          // TESTED sample after the shortcut can hang on the last bit of the position, and the sample-by-sample form below
          // keeps that bit what the reference's loop produces.
          if (n_safe > 0) walk_jump(curr, next, samp, n_safe);
          n_safe = 0;
        }
        for (; n_safe > 0; --n_safe) {
          const V3 df = sub(next, curr);
          const double dn = norm(df);
          if (!(dn > samp)) break;  // the end of the segment: the regular loop takes over
          curr = step_along(curr, samp, df, dn);
        }
      }
      continue;
    }
    V3 seed_pt = curr;  // AC:1351-1354: step back to the previous sample
    if (dist_next > 0) seed_pt = step_along(curr, -fmin(samp, dist_next), diff, dist_next);
    int seed[3];
    V3 seed_world;
    for (int ax = 0; ax < 3; ++ax) {
      seed[ax] = (int)((seed_pt[ax] - origin[ax]) / vs);
      seed_world[ax] = (seed[ax] * vs + vs / 2) + origin[ax];
    }
    bool previous_seed = false;  // AC:1361-1379
    for (int i = 0; i < n_poly; ++i)
      if (ag.polys[i].seed[0] == seed_world[0] && ag.polys[i].seed[1] == seed_world[1] && ag.polys[i].seed[2] == seed_world[2]) {
        previous_seed = true;
        break;
      }
    if (previous_seed) continue;
    int rc = HDSM_OK;
    if (c.has_world) {
      // (the local grid of this agent in world voxels, as make_window forms it)
      const hdsm_cd::WindowGrid wg = hdsm_sw::make_window(c, origin, seed, nullptr);
      const int seed_w[3] = {seed[0] + wg.ox, seed[1] + wg.oy, seed[2] + wg.oz}, off_w[3] = {wg.ox, wg.oy, wg.oz}, ground_w = wg.ground_k + wg.oz;
      const int rad = hdsm_cd::wave_map_radius(c.n_it_decomp);
      // (in x and y: the local grid is 66 voxels wide there, 20 in z — in z the growth does meet the border, so a request must come
      // from a grid at the same height; an agent changes its z voxel rarely, its x / y voxel every other round)
      const bool interior = rad > 0 && hdsm_sw::seed_in_grid(c, seed) && seed[0] - rad >= 1 && seed[1] - rad >= 1 && seed[0] + rad <= wg.lnx - 2 &&
                            seed[1] + rad <= wg.lny - 2;
      int hit = -1;
      bool hit_same_grid = false;
      if (pc != nullptr)
        for (int k = 0; k < pc->n && hit < 0; ++k) {
          const bool same_voxel = pc->seed_w[k][0] == seed_w[0] && pc->seed_w[k][1] == seed_w[1] && pc->seed_w[k][2] == seed_w[2];
          const bool same_grid = pc->off[k][0] == off_w[0] && pc->off[k][1] == off_w[1] && pc->off[k][2] == off_w[2];
          if (same_voxel && (same_grid || (interior && pc->interior[k] != 0 && pc->off[k][2] == off_w[2] && pc->ground_w[k] == ground_w))) hit = k, hit_same_grid = same_grid;
        }
      if (lane == 0 && pc != nullptr) {
        ++pc->asked;
        if (hit >= 0) ++(hit_same_grid ? pc->hits_same_grid : pc->hits_interior);
      }
      if (hit >= 0) {  // grown before from this voxel: the rows from the integers, in this grid's arithmetic
        const double org[3] = {origin[0], origin[1], origin[2]};
        const int cap = c.RS < HDSM_MAX_ROWS_STATIC ? c.RS : HDSM_MAX_ROWS_STATIC;
        const int n = hdsm_cd::rows_from_structure(pc->ps[hit], hdsm_cd::Cell{seed[0], seed[1], seed[2]}, c.voxel_size, org, lds.rows, cap);
        __syncthreads();
        if (n > cap) {
          rc = HDSM_ERR_CAPACITY, ag.polys[n_poly].rows = 0, ag.corridor_rc = rc;
        } else {
          Poly* out = &ag.polys[n_poly];
          if (lane == 0) out->rows = n;
          for (int t = lane; t < 4 * n; t += 64) {
            const int r = t >> 2, q = t & 3;
            if (q < 3) out->A[r][q] = lds.rows[t];
            else out->b[r] = lds.rows[t];
          }
          out->seed = seed_world;
        }
      } else {  // the whole wavefront, cooperatively: same arguments, same result in every lane
#if defined(CD_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
        const unsigned long long tp0 = __builtin_readcyclecounter();
#endif
        rc = world_poly_wave(c, origin, seed, lds, &ag.polys[n_poly], lane);
#if defined(CD_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
        if (lane == 0) atomicAdd(&hdsm_cd::g_cd_prof[13], __builtin_readcyclecounter() - tp0);
#endif
        if (rc != HDSM_OK) {
          ag.corridor_rc = rc;
        } else {
          ag.polys[n_poly].seed = seed_world;
          if (pc != nullptr && rad > 0) {  // (rad = 0: the plain form ran; it keeps no chamfer sources)
            int slot = pc->next;  // (a slot a map update emptied is filled first, and the ring does not move for it)
            bool hole = false;
            for (int k = 0; k < pc->n && !hole; ++k)
              if (pc->seed_w[k][0] == kCacheHole) slot = k, hole = true;
            hdsm_cd::wave_poly_structure(lds, hdsm_cd::Cell{seed[0], seed[1], seed[2]}, &pc->ps[slot], lane);
            if (lane < 3) pc->seed_w[slot][lane] = seed_w[lane], pc->off[slot][lane] = off_w[lane];
            __syncthreads();
            if (lane == 0) {
              pc->ground_w[slot] = ground_w, pc->interior[slot] = interior ? 1 : 0;
              if (!hole) pc->next = (slot + 1) % CACHE_POLYS, pc->n = pc->n < CACHE_POLYS ? pc->n + 1 : CACHE_POLYS;
            }
          }
        }
      }
    } else if (lane == 0) {
      free_space_poly(c, origin, seed, &ag.polys[n_poly]);
      ag.polys[n_poly].seed = seed_world;
    }
    __syncthreads();
    if (rc != HDSM_OK) break;
    ++n_poly;
    load_rows();
    hold_j = -1;
  }
  if (lane == 0) ag.n_poly = n_poly;
}

__device__ __attribute__((noinline)) void corridor_step_plain(const Cfg& c, AgentS& ag, hdsm_cd::Work* wk, uint32_t* bits) {
  hdsm_sw::corridor_step(c, ag, wk, bits);
}

// (the solver's inputs that do not depend on the reference — id, state, the corridor just built — leave with this kernel: a kernel
// of their own cost 5 us per round in the live loop)
__global__ __launch_bounds__(64) void k_corridor(Cfg c, int n, AgentS* agents, double* path, int32_t* n_path, int32_t* agent_id,
                                                 double* state_curr, int32_t* n_poly, int32_t* n_rows, double* A, double* b, PolyCache* cache) {
  __shared__ V3 path_s[hdsm_sw::PATH_PTS + 2];
  __shared__ V3 poly_s[PTS];
  __shared__ int np_s;
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (k >= n) return;
  AgentS& ag = agents[k];
  extern __shared__ __attribute__((aligned(16))) unsigned char slab[];  // SLAB bytes when there is a world, else none
  const hdsm_cd::WaveLds lds(slab);
  if (c.P * c.RS <= 128) {
#if defined(CD_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long tp0 = __builtin_readcyclecounter();
#endif
    corridor_step_wave(c, ag, lds, path_s, lane, cache != nullptr ? cache + k : nullptr);
#if defined(CD_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
    if (lane == 0) atomicAdd(&hdsm_cd::g_cd_prof[12], __builtin_readcyclecounter() - tp0), atomicAdd(&hdsm_cd::g_cd_prof[14], 1ull);
#endif
  } else if (lane == 0) {
    const Cfg c_call = c;  // (a copy for the call: the kernel's own stays in registers)
    corridor_step_plain(c_call, ag, lds.wk, lds.bits);  // more rows than two per lane: the plain per-agent code
  }
  __syncthreads();
  if (lane == 0) np_s = hdsm_sw::reference_polyline(ag, poly_s);
  __syncthreads();
  const int np = np_s;
  if (lane == 0) n_path[k] = np;
  for (int i = lane; i < PTS * 3; i += 64) path[(size_t)k * PTS * 3 + i] = poly_s[(i / 3) < np ? i / 3 : np - 1][i % 3];
  const int P = c.P, RS = c.RS, npo = ag.n_poly;
  if (lane < 9) state_curr[9 * (size_t)k + lane] = ag.state_curr[lane];
  if (lane == 0) agent_id[k] = ag.id, n_poly[k] = npo;
  if (lane < P) n_rows[(size_t)k * P + lane] = lane < npo ? ag.polys[lane].rows : 0;
  for (int t = lane; t < P * RS; t += 64) {
    const int j = t / RS, r = t % RS;
    const bool hr = j < npo && r < ag.polys[j].rows;
    for (int q = 0; q < 3; ++q) A[((size_t)k * P * RS + t) * 3 + q] = hr ? ag.polys[j].A[r][q] : 0.0;
    b[(size_t)k * P * RS + t] = hr ? ag.polys[j].b[r] : 0.0;
  }
}

// the map-dependent half of the reference (row f1 remainder): ComputePathVelocity's voxel term before k_reference ...
__global__ __launch_bounds__(64) void k_vel_cap(Cfg c, hdsm_ref_config rc, int n, const AgentS* agents, const double* path, const int32_t* n_path,
                                                double* vel_cap) {
  // one wavefront per agent, one path segment per lane (two ray casts each): the reference stops at the first segment that collides,
  // i.e. the cap is the minimum over the segments up to and including that one
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (k >= n) return;
  const int np = n_path[k];
  double cap = rc.path_vel_max;
  if (c.has_world && np >= 1) {
    const V3 origin = hdsm_sw::local_grid_origin(c, agents[k]);
    const hdsm_sw::RawWindow g = hdsm_sw::raw_window(c, origin);
    auto pt = [&](int i) { return V3{{path[((size_t)k * PTS + i) * 3], path[((size_t)k * PTS + i) * 3 + 1], path[((size_t)k * PTS + i) * 3 + 2]}}; };
    const V3 p0 = pt(0);
    for (int base = 0; base + 1 < np; base += 64) {  // (PTS <= 64 segments in practice: one trip)
      const int i = base + lane;
      bool collided = false;
      double v = rc.path_vel_max;
      if (i + 1 < np) v = hdsm_sw::voxel_velocity_cap_segment(c, rc, g, origin, p0, pt(i), pt(i + 1), &collided);
      const unsigned long long hit = __ballot(collided);
      const int first = hit != 0ull ? __ffsll((long long)hit) - 1 : 64;
      if (lane > first) v = rc.path_vel_max;
      for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
      cap = fmin(cap, v);
      if (hit != 0ull) break;
    }
  }
  if (lane == 0) vel_cap[k] = cap;
}

// ... and KeepOnlyFreeReference (AC:1665-1693) after it, on the rows k_reference wrote
__global__ __launch_bounds__(64) void k_keep_free(Cfg c, int n, const AgentS* agents, double* ref_full, double* ref, const double* path_vel) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n) return;
  const int N = c.N;
  double rows[hdsm::MAXH + 1][6];
  for (int i = 0; i <= N; ++i)
    for (int q = 0; q < 6; ++q) rows[i][q] = ref_full[((size_t)k * (N + 1) + i) * 6 + q];
  hdsm_sw::keep_only_free(c, hdsm_sw::local_grid_origin(c, agents[k]), path_vel[k], rows, N + 1);
  for (int i = 0; i <= N; ++i)
    for (int q = 0; q < 6; ++q) {
      ref_full[((size_t)k * (N + 1) + i) * 6 + q] = rows[i][q];
      if (i < N) ref[((size_t)k * N + i) * 6 + q] = rows[i][q];
    }
}

__global__ __launch_bounds__(64) void k_commit(Cfg c, int n, int per, AgentS* agents, const double* traj, const double* ctrl,
                                               const uint8_t* used, const int32_t* status, double* plans_local, int32_t* fails,
                                               uint8_t* has_direct, const double* ref_full, const double* path_vel) {
  // one wavefront per published record. Lane 0 does the read-back / fallback; the increment check — a walk of ~100 samples per
  // metre of reference — is split by reference segment over the lanes (the samples of a segment do not depend on the others,
  // hdsm_sw::increment_segment_min), the minima meet in a wave reduction; then all lanes write the record.
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (k >= per) return;
  const int N = c.N, rec = (N + 1) * 9;
  double* out = plans_local + (size_t)k * rec;
  __shared__ int have_s;
  if (lane == 0) have_s = 0;
  __syncthreads();
  if (k < n) {
    AgentS& ag = agents[k];
    // the reference of this round becomes traj_ref_curr_ (the increment check below and the next round's corridor read it)
    for (int t = lane; t < (N + 1) * 6; t += 64) ag.traj_ref[t / 6][t % 6] = ref_full[(size_t)k * (N + 1) * 6 + t];
    if (lane == 0) ag.n_ref = N + 1, ag.path_vel = path_vel[k];
    {  // hdsm_sw::commit_copy with the copies spread over the lanes (one lane doing them was a chain of ~130 dependent
       // global accesses, 35 of the kernel's 40 us): flat element e of traj_curr[][9] / ctrl_curr[][3]
      const int st = status[k];
      double* tc = &ag.traj_curr[0][0];
      double* cc = &ag.ctrl_curr[0][0];
      if (st != HDSM_NO_SOLUTION) {  // AC:960-987
        const double* tin = traj + (size_t)k * rec;
        const double* cin = ctrl + (size_t)k * N * 3;
        for (int e = lane; e < rec; e += 64) tc[e] = tin[e];
        for (int e = lane; e < N * 3; e += 64) cc[e] = cin[e];
        if (lane < c.P) ag.poly_used[lane] = used[(size_t)k * c.P + lane];
        if (lane == 0) ag.has_traj = 1, have_s = 1;
      } else {  // AC:1000-1019: every lane reads what it moves before anybody writes
        constexpr int PER = (hdsm::MAXH * 9 + 63) / 64;
        const bool shift = ag.has_traj != 0;
        double tv[PER], cv[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
          const int e = lane + 64 * u;
          tv[u] = (shift && e < N * 9) ? tc[e + 9] : 0.0;
          cv[u] = (shift && e < (N - 1) * 3) ? cc[e + 3] : 0.0;
        }
        __syncthreads();
        if (shift) {
#pragma unroll
          for (int u = 0; u < PER; ++u) {
            const int e = lane + 64 * u;
            if (e < N * 9) tc[e] = tv[u];
            if (e < (N - 1) * 3) cc[e] = cv[u];
          }
        }
        if (lane == 0) {
          ++ag.n_fail;
          atomicAdd(fails, 1);
          have_s = shift ? 1 : 0;
        }
      }
    }
    __syncthreads();
    if (have_s) {
      int inc = 0;
      if (ag.n_ref >= 2) {
        const V3 pt = {{ag.traj_curr[1][0], ag.traj_curr[1][1], ag.traj_curr[1][2]}};
        const double d0 = hdsm_sw::norm(hdsm_sw::sub(pt, V3{{ag.traj_ref[0][0], ag.traj_ref[0][1], ag.traj_ref[0][2]}}));
        // The minimum over the samples in closed form first (three candidate samples per segment instead of ~90 generated one
        // after the other, two square roots and three divisions in a chain each: half of this kernel's time). It differs from
        // the literal walk's minimum by ~1e-11 m at most; the decision compares the minimum with d0 and thresh_dist, so unless one
        // of those comparisons is closer than 1e-9 m the literal walk would decide the same — and when one is, it is walked.
        double best = DBL_MAX;
        if (lane < ag.n_ref - 1) best = hdsm_sw::increment_segment_min_closed_form(ag, lane, pt);
        for (int off = 32; off > 0; off >>= 1) best = fmin(best, __shfl_xor(best, off));
        // (the literal walk's accumulated rounding is ~100 steps x ulp(position): the guard grows with the magnitude of the
        // coordinates, 1e-9 m up to a few hundred metres, so that worlds of 1e5 m keep the same safety factor)
        const double mag = fmax(fmax(fabs(pt.v[0]), fabs(pt.v[1])), fabs(pt.v[2]));
        const double guard = 1e-9 * fmax(1.0, mag * 0.01);
        if (!(fabs(best - d0) > guard && fabs(best - c.thresh_dist) > guard)) {
          best = DBL_MAX;
          if (lane < ag.n_ref - 1) best = hdsm_sw::increment_segment_min(ag, lane, pt);
          for (int off = 32; off > 0; off >>= 1) best = fmin(best, __shfl_xor(best, off));
        }
        inc = hdsm_sw::increment_from_minima(c, d0, best);
      }
      if (lane == 0) ag.increment = inc;
      if (lane < 9) ag.state_curr[lane] = ag.traj_curr[c.step_plan][lane];  // AC:233-238
      for (int e = lane; e < rec; e += 64) out[e] = ag.traj_curr[e / 9][e % 9];
    }
  }
  if (!have_s) {  // no plan yet (or padding): the record carries the sentinel instead of a flag (hdsm_exchange_device)
    for (int e = lane; e < rec; e += 64) out[e] = e == 0 ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
  }
  // a single rank publishes straight into the plans buffer of the next round (no copy, no flag kernel): the flag too
  if (has_direct != nullptr && lane == 0) has_direct[k] = have_s ? 1 : 0;
}

// Agent::UpdatePath (AC:261-454) by the rule of path_core.h, ONE WORKGROUP PER DUE AGENT (idx: the due agents, NULL = all n):
// the BFS as bit planes in LDS (hdsm_path::plan_block), the same points as the host mirror's hdsm_path::plan_serial. goals[k]
// (hdsm_dswarm_set_goals) becomes the agent's goal first. cnt[0] agents planned, cnt[1] failed.
__global__ __launch_bounds__(hdsm_path::THREADS) void k_path(Cfg c, const int32_t* idx, AgentS* agents, const double* goals,
                                                              unsigned long long* cnt) {
  __shared__ hdsm_path::PathLds lds;
  const int tid = (int)threadIdx.x;
  const int k = idx != nullptr ? idx[blockIdx.x] : (int)blockIdx.x;
  AgentS& ag = agents[k];
  const V3 goal = {{goals[3 * (size_t)k], goals[3 * (size_t)k + 1], goals[3 * (size_t)k + 2]}};
  const hdsm_path::PathIn in = hdsm_path::agent_problem(c, ag, goal);
  const int st = hdsm_path::plan_block(in, lds, tid);
  __syncthreads();  // (every thread has read the agent's state)
  const int n = lds.n_out;
  if (tid == 0) {
    ag.goal = goal, ag.path_rc = st;
    if (st == hdsm_path::PATH_OK) ag.n_path = n;
    atomicAdd(&cnt[0], 1ull);
    if (st != hdsm_path::PATH_OK) atomicAdd(&cnt[1], 1ull);
  }
  if (st == hdsm_path::PATH_OK)
    for (int t = tid; t < 3 * n; t += hdsm_path::THREADS) ag.path[t / 3][t % 3] = lds.out[t / 3][t % 3];
}

// k_path in clearance mode (path_core.h, 6a-7': the distance-map planner and ShortenDMPPath after the descent); rn, rows: the tunnel's
// mask (hdsm_path::DmpMask). The same bookkeeping as k_path.
__global__ __launch_bounds__(hdsm_path::THREADS) void k_dmp(Cfg c, const int32_t* idx, AgentS* agents, const double* goals,
                                                             unsigned long long* cnt, int rn, const uint32_t* rows) {
  __shared__ hdsm_path::DmpLds lds;
  const int tid = (int)threadIdx.x;
  const int k = idx != nullptr ? idx[blockIdx.x] : (int)blockIdx.x;
  AgentS& ag = agents[k];
  const V3 goal = {{goals[3 * (size_t)k], goals[3 * (size_t)k + 1], goals[3 * (size_t)k + 2]}};
  const hdsm_path::PathIn in = hdsm_path::agent_problem(c, ag, goal);
  const int st = hdsm_path::plan_dmp_block(in, rn, rows, lds, tid);
  __syncthreads();  // (every thread has read the agent's state)
  const int n = lds.p.n_out;
  if (tid == 0) {
    ag.goal = goal, ag.path_rc = st;
    if (st == hdsm_path::PATH_OK) ag.n_path = n;
    atomicAdd(&cnt[0], 1ull);
    if (st != hdsm_path::PATH_OK) atomicAdd(&cnt[1], 1ull);
  }
  if (st == hdsm_path::PATH_OK)
    for (int t = tid; t < 3 * n; t += hdsm_path::THREADS) ag.path[t / 3][t % 3] = lds.p.out[t / 3][t % 3];
}

// ---- map updates in flight (ABI 1.7) ----
// values [bdim[2]][bdim[1]][bdim[0]] into the box lo .. lo + bdim of a grid [.][ny][nx]: thread <-> up to four voxels of one row
__global__ __launch_bounds__(256) void k_box_put(const int8_t* __restrict__ vals, int8_t* __restrict__ grid, int nx, int ny, int lx, int ly, int lz,
                                                 int bx, int by, int bz) {
  const int qpr = (bx + 3) / 4, rows = by * bz;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < qpr * rows; q += gridDim.x * blockDim.x) {
    const int row = q / qpr, x0 = (q - row * qpr) * 4, z = row / by, y = row - z * by;
    const int n = bx - x0 < 4 ? bx - x0 : 4;
    const int8_t* in = vals + (size_t)row * bx + x0;
    int8_t* out = grid + ((size_t)(lz + z) * ny + (ly + y)) * nx + (lx + x0);
    if (n == 4) __builtin_memcpy(out, in, 4);
    else
      for (int k = 0; k < n; ++k) out[k] = in[k];
  }
}

// The polyhedron cache after voxels lo .. hi (inclusive, world voxels) were written: one lane per (agent, entry). An entry whose
// decomposition could have looked at a written voxel — its seed +- (rad + 1): wave_map_radius and one voxel of margin — is dropped,
// the others stay. A dropped entry becomes a hole: its seed voxel is set to kCacheHole, so it is never found again, and the agent's
// n / next are left as they are; the next polyhedron k_corridor records goes into the first hole, so the agent keeps its six slots.
// (An entry is read only through the comparison of its seed voxel, so nothing else of it needs clearing.)
__global__ __launch_bounds__(256) void k_cache_invalidate(PolyCache* cache, int n_agents, int rad, int lx, int ly, int lz, int hx, int hy, int hz,
                                                          unsigned long long* dropped) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_agents * CACHE_POLYS) return;
  PolyCache& pc = cache[t / CACHE_POLYS];
  const int e = t % CACHE_POLYS;
  if (e >= pc.n || pc.seed_w[e][0] == kCacheHole) return;
  const int sx = pc.seed_w[e][0], sy = pc.seed_w[e][1], sz = pc.seed_w[e][2];
  const bool meets = sx + rad >= lx && sx - rad <= hx && sy + rad >= ly && sy - rad <= hy && sz + rad >= lz && sz - rad <= hz;
  if (!meets) return;
  pc.seed_w[e][0] = kCacheHole;
  atomicAdd(dropped, 1ull);
}

using hdsm_mem::DevBuf;

// the path step (k_path): period and round phase of the host mirror, the agents due at the next round (hdsm_dswarm_set_goals) and
// their list on the device, every agent's goal (host copy + device), counters [planned, failed], launches, the timed interval
struct PathStep {
  int period = 0;
  long long round = 0, launches = 0;
  std::vector<uint8_t> due;
  std::vector<double> goals;
  int n_due = 0;
  DevBuf<int32_t> d_due;
  DevBuf<double> d_goals;
  DevBuf<unsigned long long> d_cnt;
  hdsm_mem::TimedInterval timed;
  // the clearance mode (hdsm_swarm_set_path_clearance before hdsm_dswarm_create): k_dmp instead of k_path, the mask's rows on the device
  bool dmp = false;
  int dmp_rn = 0;
  DevBuf<uint32_t> d_dmp_rows;
};

// the flight audit (audit_kernels.hip; opt-in: nothing is allocated or launched while it and the history are off)
struct Audit {
  bool on = false, ever = false;
  long long rounds = 0;  // rounds audited by this dswarm (hdsm_dswarm_last_audit_round needs one)
  double sep_warn = 1.0;
  hdsm_audit::DeviceBufs buf;
  DevBuf<hdsm_flight_report> d_report;
  hdsm_mem::TimedInterval timed;  // the audit's launches of a round, the history write included
};

// the state history (opt-in, written by the audit's last kernel): rows [cap][n_local][9]
struct History {
  DevBuf<double> d_rows;
  int cap = 0, n = 0, dropped = 0, delivered = 0;
  bool last = false;  // the last round wrote row n - 1 (a state taken from outside behind that round replaces the agent's entry of it)
};

// map updates in flight (nothing is allocated or launched before the first hdsm_dswarm_update_world* / _set_raw_world): the
// resident raw grid with the map configuration and the scratch of the region pre-processing, the staging buffer of the
// host-pointer forms, updates applied, voxels written, and the device's count of cache entries dropped
struct WorldEdits {
  DevBuf<int8_t> d_raw;
  DevBuf<uint8_t> d_map_scr;
  hdsm_map_config mcfg{};
  DevBuf<int8_t> d_edit;
  size_t edit_cap = 0;
  long long updates = 0, voxels = 0;
  DevBuf<unsigned long long> d_dropped;
};

// link faults (hdsm_dswarm_set_links; nothing is allocated or launched before the first call): the fate table, the ring of the last
// rounds' published records ([MAX_DELAY + 1][G][rec], allocated once at the longest a table may ask for; D + 1 of them are in use),
// the view the next round's reference and solve read in place of the plans buffer, and the per-slot counters
struct Links {
  bool on = false;
  int n_rounds = 0, D = 0, time_aware = 0;
  int round = 0;  // the link round the next k_deliver closes (0: the first round after hdsm_dswarm_set_links)
  hdsm_mem::GrowBuf<int8_t> d_fate;
  DevBuf<double> d_ring, d_seen;
  DevBuf<uint8_t> d_seen_has;
  DevBuf<int32_t> d_seen_round, d_shift, d_cnt;
  bool ready() const { return (bool)d_cnt; }
};

// scripted agents (hdsm_dswarm_set_script; nothing is allocated or launched before the first call that scripts somebody): the LAST n
// ids of the shard's block are not flown — every kernel in front of k_commit runs on the n_local - n agents before them — and k_script
// publishes their records from the tracks ([n_local][MAX_KNOTS][4] on the device, allocated once; n x n_knots of them in use).
struct Script {
  int n = 0, n_knots = 0, predict = 0;
  long long round = 0;  // the script round the next k_script publishes (0: the first round after hdsm_dswarm_set_script)
  long long launches = 0;
  DevBuf<double> d_knots;
};

// imperfect tracking (hdsm_dswarm_set_tracking / _set_states*; nothing is allocated or launched before the first call that needs it): the
// model while it is on, the tracking round the next k_track flies, the launches of the two forms, the record per agent ([n_local],
// zeros at first) and the staging of the host-pointer form of a state from outside
struct Track {
  bool on = false;
  hdsm_tracking model{};
  long long q = 0, model_launches = 0, external_launches = 0;
  DevBuf<hdsm_track_record> d_rec;
  DevBuf<double> d_stage;
  DevBuf<uint8_t> d_stage_mask;
};

// One link round (link_core.h, deliver_slot): a wavefront per slot of the plans buffer, four per workgroup. No LDS, no atomics: a
// slot is touched by its own wavefront alone.
__global__ __launch_bounds__(256) void k_deliver(hdsm_link::Round a) {
  const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (k >= a.G) return;
  hdsm_link::deliver_slot(a, k, (int)threadIdx.x & 63, 64);
}

// ---- neighbour groups: the per-group flight summary (hdsm_dswarm_group_report) ----
// One wavefront per group over the group's LOCAL agents [max(lo, first), min(hi, first + n_local)), 64 at a time; groups larger than
// a wavefront loop. Every figure is an integer sum, a minimum or a maximum, reduced over the wave by butterflies: the result does not
// depend on the order. The separation minimum orders (sep2_min, agent id) — a total order: ties go to the lower agent id. No atomics,
// no LDS. report == nullptr (the audit was never on): the audit fields are zeros and -1. With the audit on, a group without a pair
// (one agent) has sep2_min = DBL_MAX and sep_agent = -1, as in an empty hdsm_flight_report.
template <class T>
__device__ __forceinline__ T wave_xor(T v, int m) {
  return __shfl_xor(v, m, 64);
}
__global__ __launch_bounds__(64) void k_group_report(int first, int n_local, const int32_t* __restrict__ gstart, const AgentS* __restrict__ agents,
                                                     const int32_t* __restrict__ status, const hdsm_flight_report* __restrict__ report,
                                                     hdsm_group_report* __restrict__ out) {
  const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int lo = gstart[g], hi = gstart[g + 1];
  const int l0 = lo > first ? lo : first, l1 = hi < first + n_local ? hi : first + n_local;
  long long no_sol = 0, failed = 0, rounds = 0, positions = 0, close_r = 0, occupied = 0, unknown = 0, crossed = 0, pot = 0;
  double dist_goal = 0.0, speed_max = 0.0, q = DBL_MAX;
  int q_agent = -1, q_partner = -1, q_sub = 0;
  long long q_round = -1;
  for (int a = l0 + lane; a < l1; a += 64) {
    const int k = a - first;
    const AgentS& ag = agents[k];
    no_sol += status[k] == HDSM_NO_SOLUTION, failed += ag.n_fail;
    const double dg = hdsm_sw::norm(hdsm_sw::sub(V3{{ag.state_curr[0], ag.state_curr[1], ag.state_curr[2]}}, ag.goal));
    dist_goal = dg > dist_goal ? dg : dist_goal;
    if (report != nullptr) {
      const hdsm_flight_report r = report[k];
      rounds = r.rounds > rounds ? r.rounds : rounds;
      positions += r.positions, close_r += r.close_rounds, occupied += r.occupied, unknown += r.unknown, crossed += r.crossed, pot += r.pot_sum;
      speed_max = r.speed_max > speed_max ? r.speed_max : speed_max;
      if (r.sep_partner >= 0 && (q_agent < 0 || r.sep2_min < q))  // (ids ascend within a lane: '<' keeps the lower one)
        q = r.sep2_min, q_agent = a, q_partner = r.sep_partner, q_sub = r.sep_substep, q_round = r.sep_round;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    no_sol += wave_xor(no_sol, m), failed += wave_xor(failed, m), positions += wave_xor(positions, m), close_r += wave_xor(close_r, m);
    occupied += wave_xor(occupied, m), unknown += wave_xor(unknown, m), crossed += wave_xor(crossed, m), pot += wave_xor(pot, m);
    const long long o_rounds = wave_xor(rounds, m);
    rounds = o_rounds > rounds ? o_rounds : rounds;
    const double o_dg = wave_xor(dist_goal, m), o_sp = wave_xor(speed_max, m);
    dist_goal = o_dg > dist_goal ? o_dg : dist_goal, speed_max = o_sp > speed_max ? o_sp : speed_max;
    const double o_q = wave_xor(q, m);
    const int o_agent = wave_xor(q_agent, m), o_partner = wave_xor(q_partner, m), o_sub = wave_xor(q_sub, m);
    const long long o_round = wave_xor(q_round, m);
    if (o_agent >= 0 && (q_agent < 0 || o_q < q || (o_q == q && o_agent < q_agent)))
      q = o_q, q_agent = o_agent, q_partner = o_partner, q_sub = o_sub, q_round = o_round;
  }
  if (lane == 0) {
    hdsm_group_report r;
    r.first = lo, r.count = hi - lo, r.n_local = l1 > l0 ? l1 - l0 : 0, r.no_solution_last = (int32_t)no_sol;
    r.failed_total = failed, r.dist_goal_max = dist_goal;
    r.rounds = rounds, r.positions = positions, r.close_rounds = close_r, r.occupied = occupied, r.unknown = unknown, r.crossed = crossed;
    r.pot_sum = pot, r.sep2_min = report != nullptr ? q : 0.0, r.sep_agent = q_agent, r.sep_partner = q_partner, r.sep_substep = q_sub, r.reserved0 = 0;
    r.sep_round = q_round, r.speed_max = speed_max;
    out[g] = r;
  }
}

struct DSwarm {
  void* solver = nullptr;
  int device = 0, n_local = 0, n_rob = 0, first = 0, per = 0, world = 1;
  hdsm_params prm{};
  hdsm_swarm_config cfg{};
  hdsm_ref_config rcfg{};
  Cfg c{};
  DevBuf<AgentS> d_agents;
  DevBuf<PolyCache> d_cache;  // [n_local], worlds only (HDSM_POLY_CACHE=0: none)
  DevBuf<int8_t> d_world;
  DevBuf<double> d_cap, d_path, d_ref_full, d_ref, d_pv, d_state, d_A, d_b, d_traj, d_ctrl, d_obj, d_local, d_plans;
  DevBuf<int32_t> d_npath, d_id, d_npoly, d_nrows, d_status, d_fails;
  DevBuf<uint8_t> d_used, d_has;
  long long rounds = 0;
  // hdsm_dswarm_set_phase_timing: HIP events between the launches of a round (development / bench aid: every record is a barrier
  // packet in front of the next kernel, so a timed round is a few us longer than a plain one — ms_per_round is never taken from it)
  bool phase_timing = false, phase_valid = false;
  hdsm_mem::DevEvent ev[8];
  PathStep path;
  Audit audit;
  History hist;
  WorldEdits edits;
  Links links;
  Script script;
  Track track;
  int n_fly() const { return n_local - script.n; }  // the agents this shard plans for: all but its scripted tail
  // neighbour groups (taken from the mirror by hdsm_dswarm_create; one group = the whole swarm without a partition): the
  // partition, the id range per record of the plans buffer ([per * world][2], for the audit; null without a partition), the report
  std::vector<int32_t> group_start;
  bool grouped = false;
  DevBuf<int32_t> d_gstart, d_range;
  DevBuf<hdsm_group_report> d_greport;
};

// every event a timed round records (hdsm_dswarm_set_phase_timing; _set_audit and _set_history when the timing is already on)
int timing_events(DSwarm* d) {
  for (hdsm_mem::DevEvent& e : d->ev) HIP_TRY(e.create());
  HIP_TRY(d->path.timed.create());
  HIP_TRY(d->audit.timed.create());
  return HDSM_OK;
}

// the audit's scratch and (at the first switch-on) the flight record of the shard; `init` [n_local] or empty reports
int audit_setup(DSwarm* d, const hdsm_flight_report* init) {
  Audit& a = d->audit;
  if (!a.buf.d_round) {
    if (hdsm_audit::device_alloc(&a.buf, d->per * d->world, d->n_local, d->c.step_plan) != hipSuccess)
      return fail(HDSM_ERR_DEVICE, "flight audit: allocation failed");
  }
  if (!a.d_report && (init != nullptr || a.on)) {
    std::vector<hdsm_flight_report> rep((size_t)d->n_local);
    for (int k = 0; k < d->n_local; ++k) {
      if (init) rep[k] = init[k];
      else hdsm_audit::empty_report(&rep[k]);
    }
    HIP_TRY(a.d_report.alloc(rep.size() + 1));
    if (!rep.empty()) HIP_TRY(hipMemcpy(a.d_report.get(), rep.data(), rep.size() * sizeof(hdsm_flight_report), hipMemcpyHostToDevice));
    a.ever = true;
  }
  return HDSM_OK;
}

// the box lo .. lo + bdim inside the device world? (0 empty, 1 yes, < 0 an error)
int world_box(DSwarm* d, const int32_t* lo, const int32_t* bdim) {
  if (!d || !lo || !bdim) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return fail(HDSM_ERR_BAD_ARG, "the dswarm has no world (hdsm_swarm_set_world before hdsm_dswarm_create)");
  for (int ax = 0; ax < 3; ++ax)
    if (bdim[ax] < 0 || lo[ax] < 0 || lo[ax] > d->c.wdim[ax] || bdim[ax] > d->c.wdim[ax] - lo[ax])
      return fail(HDSM_ERR_BAD_ARG, "the box does not lie inside the world");
  return (bdim[0] == 0 || bdim[1] == 0 || bdim[2] == 0) ? 0 : 1;
}

// values (device) into the box of `grid` (the device world or the resident raw grid), on st
int put_box(DSwarm* d, const int8_t* d_vals, int8_t* grid, const int32_t lo[3], const int32_t bdim[3], hipStream_t st) {
  const int quads = ((bdim[0] + 3) / 4) * bdim[1] * bdim[2];
  hipLaunchKernelGGL(k_box_put, dim3((unsigned)std::min((quads + 255) / 256, 4096)), dim3(256), 0, st, d_vals, grid, d->c.wdim[0], d->c.wdim[1], lo[0],
                     lo[1], lo[2], bdim[0], bdim[1], bdim[2]);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

// drops the cache entries that could have looked at the written voxels wlo .. wlo + wdim (NULL: every entry), on st, and books the update
int invalidate(DSwarm* d, const int32_t* wlo, const int32_t* wdim, hipStream_t st) {
  if (!d->edits.d_dropped) HIP_TRY(d->edits.d_dropped.alloc_zeroed(1));
  if (!d->d_cache || d->n_local == 0) return HDSM_OK;
  const int rad = hdsm_cd::wave_map_radius(d->c.n_it_decomp) + 1;
  const int big = 1 << 29;
  const int l[3] = {wlo ? wlo[0] : -big, wlo ? wlo[1] : -big, wlo ? wlo[2] : -big};
  const int h[3] = {wlo ? wlo[0] + wdim[0] - 1 : big, wlo ? wlo[1] + wdim[1] - 1 : big, wlo ? wlo[2] + wdim[2] - 1 : big};
  hipLaunchKernelGGL(k_cache_invalidate, dim3((unsigned)((d->n_local * CACHE_POLYS + 255) / 256)), dim3(256), 0, st, d->d_cache.get(), d->n_local, rad, l[0],
                     l[1], l[2], h[0], h[1], h[2], d->edits.d_dropped.get());
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

// the host values of a box into the staging buffer (the device is idle: the callers have synchronised)
int stage_box(DSwarm* d, const int8_t* values, const int32_t bdim[3]) {
  WorldEdits& w = d->edits;
  const size_t bytes = (size_t)bdim[0] * bdim[1] * bdim[2];
  if (bytes > w.edit_cap) {
    w.edit_cap = 0;
    HIP_TRY(w.d_edit.alloc(bytes));
    w.edit_cap = bytes;
  }
  HIP_TRY(hipMemcpy(w.d_edit.get(), values, bytes, hipMemcpyHostToDevice));
  return HDSM_OK;
}

// every buffer a round of n_local agents in a world of hworld's size needs, zero-filled
hipError_t alloc_round_buffers(DSwarm* d, const int8_t* hworld) {
  const Cfg& c = d->c;
  const size_t n = (size_t)d->n_local, L = (size_t)d->per, G = (size_t)d->per * d->world, N = (size_t)c.N, P = (size_t)c.P, RS = (size_t)c.RS,
               REC = (N + 1) * 9;
  hdsm_mem::FirstError ok;
  ok(d->d_agents.alloc_zeroed(n));
  if (hworld) {
    ok(d->d_world.alloc_zeroed((size_t)c.wdim[0] * c.wdim[1] * c.wdim[2]));
    bool cache_on = true;  // development switch (A/B): HDSM_POLY_CACHE=0 grows every polyhedron again
    if (const char* pcenv = std::getenv("HDSM_POLY_CACHE")) cache_on = !(pcenv[0] == '0' && pcenv[1] == 0);
    if (cache_on) ok(d->d_cache.alloc_zeroed(n));
  }
  ok(d->d_path.alloc_zeroed(n * PTS * 3)), ok(d->d_npath.alloc_zeroed(n)), ok(d->d_ref_full.alloc_zeroed(n * (N + 1) * 6));
  ok(d->d_ref.alloc_zeroed(n * N * 6)), ok(d->d_cap.alloc_zeroed(n)), ok(d->d_pv.alloc_zeroed(n)), ok(d->d_id.alloc_zeroed(n));
  ok(d->d_state.alloc_zeroed(n * 9)), ok(d->d_npoly.alloc_zeroed(n)), ok(d->d_nrows.alloc_zeroed(n * P));
  ok(d->d_A.alloc_zeroed(n * P * RS * 3)), ok(d->d_b.alloc_zeroed(n * P * RS)), ok(d->d_traj.alloc_zeroed(L * REC));
  ok(d->d_ctrl.alloc_zeroed(L * N * 3)), ok(d->d_obj.alloc_zeroed(L)), ok(d->d_used.alloc_zeroed(L * P)), ok(d->d_status.alloc_zeroed(L));
  ok(d->d_local.alloc_zeroed(L * REC)), ok(d->d_plans.alloc_zeroed(G * REC)), ok(d->d_has.alloc_zeroed(G)), ok(d->d_fails.alloc_zeroed(1));
  ok(d->path.d_due.alloc_zeroed(n)), ok(d->path.d_goals.alloc_zeroed(n * 3)), ok(d->path.d_cnt.alloc_zeroed(2));
  return ok.e;
}

// The mirror's flight becomes the device's (hdsm_dswarm_create, after alloc_round_buffers): the path step's phase and pending agents,
// the clearance mode, the agent states, ids and goals, the world (hworld: the mirror's grid or NULL), the audit's setting and record.
int take_over(DSwarm& d, void* swarm, const int8_t* hworld) {
  const size_t n = (size_t)d.n_local;
  PathStep& p = d.path;
  const auto refused = [](int rc) { return fail(rc, "hdsm_dswarm_create: export failed"); };
  p.due.assign(n, 0), p.goals.assign(n * 3, 0.0);
  int32_t period = 0;
  int64_t round = 0;
  if (int rc = hdsm_swarm_export_path_state(swarm, &period, &round, p.due.data())) return refused(rc);
  p.period = period, p.round = round;
  double rad = 0;
  if (int rc = hdsm_swarm_export_path_clearance(swarm, &rad)) return refused(rc);
  if (rad != 0) {
    hdsm_path::DmpMask mask{};
    if (!hdsm_path::dmp_build_mask(rad, d.cfg.voxel_size, &mask)) return refused(HDSM_ERR_BAD_ARG);
    p.dmp = true, p.dmp_rn = mask.rn;
    HIP_TRY(p.d_dmp_rows.alloc_zeroed(sizeof mask.rows / sizeof mask.rows[0]));
    HIP_TRY(hipMemcpy(p.d_dmp_rows.get(), mask.rows, sizeof mask.rows, hipMemcpyHostToDevice));
  }
  if (n) {
    std::unique_ptr<AgentS[]> tmp(new (std::nothrow) AgentS[n]);
    if (!tmp) return fail(HDSM_ERR_DEVICE, "out of host memory");
    if (int rc = hdsm_swarm_export_state(swarm, tmp.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return refused(rc);
    HIP_TRY(hipMemcpy(d.d_agents.get(), tmp.get(), n * sizeof(AgentS), hipMemcpyHostToDevice));
    // the agent ids of the shard (a contiguous block), the goals, and the agents the mirror had marked due (hdsm_swarm_set_goals before the dswarm)
    std::vector<int32_t> ids(n, 0), idx;
    for (size_t k = 0; k < n; ++k) {
      for (int q = 0; q < 3; ++q) p.goals[3 * k + q] = tmp[k].goal[q];
      ids[k] = d.first + (int)k;
      if (p.due[k]) idx.push_back((int32_t)k);
    }
    p.n_due = (int)idx.size();
    HIP_TRY(hipMemcpy(d.d_id.get(), ids.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.d_goals.get(), p.goals.data(), n * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (p.n_due) HIP_TRY(hipMemcpy(p.d_due.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (hworld) HIP_TRY(hipMemcpy(d.d_world.get(), hworld, (size_t)d.c.wdim[0] * d.c.wdim[1] * d.c.wdim[2], hipMemcpyHostToDevice));
  d.c.world = d.d_world.get();
  {  // the mirror's partition goes onto the solver handle (none: the handle's is cleared) and, for the audit, into a range table
    int32_t ng = 0;
    if (int rc = hdsm_swarm_export_groups(swarm, &ng, nullptr)) return refused(rc);
    d.grouped = ng > 0;
    d.group_start.assign((size_t)(d.grouped ? ng + 1 : 2), 0);
    if (d.grouped) {
      if (int rc = hdsm_swarm_export_groups(swarm, &ng, d.group_start.data())) return refused(rc);
    } else {
      d.group_start[1] = d.n_rob;
    }
    if (int rc = hdsm_set_groups(d.solver, d.grouped ? ng : 0, d.grouped ? d.group_start.data() : nullptr))
      return fail(rc, std::string("hdsm_set_groups: ") + hdsm_last_error());
    HIP_TRY(hipSetDevice(d.device));  // (the handle may live on another device)
    if (d.grouped) {
      const size_t G = (size_t)d.per * d.world;
      std::vector<int32_t> table(2 * G + 2, 0);
      for (int g = 0; g < ng; ++g)
        for (int k = d.group_start[g]; k < d.group_start[g + 1]; ++k) table[2 * (size_t)k] = d.group_start[g], table[2 * (size_t)k + 1] = d.group_start[g + 1];
      HIP_TRY(d.d_range.alloc(table.size()));
      HIP_TRY(hipMemcpy(d.d_range.get(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
  }
  int32_t on = 0, ever = 0;  // the audit's setting and record of the mirror (a flight taken over keeps its record)
  if (int rc = hdsm_swarm_export_audit(swarm, &on, &ever, &d.audit.sep_warn, nullptr)) return refused(rc);
  if (ever) {
    std::vector<hdsm_flight_report> rep(n);
    if (int rc = hdsm_swarm_export_audit(swarm, &on, &ever, &d.audit.sep_warn, rep.data())) return refused(rc);
    d.audit.on = on != 0;
    if (int rc = audit_setup(&d, rep.data())) return rc;
  }
  return HDSM_OK;
}

// The device's flight back into the mirror (hdsm_dswarm_download; the device is idle): the agent states, the path step's phase,
// pending agents and goals, the audit's setting and record.
int hand_back(DSwarm& d, void* swarm) {
  const size_t n = (size_t)d.n_local;
  std::unique_ptr<AgentS[]> tmp(new (std::nothrow) AgentS[n]);
  if (!tmp) return fail(HDSM_ERR_DEVICE, "out of host memory");
  int rc = hipMemcpy(tmp.get(), d.d_agents.get(), n * sizeof(AgentS), hipMemcpyDeviceToHost) == hipSuccess
               ? hdsm_swarm_import_state(swarm, tmp.get(), d.n_local)
               : HDSM_ERR_DEVICE;
  if (rc == HDSM_OK) rc = hdsm_swarm_import_path_state(swarm, d.path.period, d.path.round, d.path.due.data(), d.path.goals.data());
  if (rc == HDSM_OK && d.audit.ever) {
    std::vector<hdsm_flight_report> rep(n);
    if (hipMemcpy(rep.data(), d.audit.d_report.get(), n * sizeof(hdsm_flight_report), hipMemcpyDeviceToHost) != hipSuccess) rc = HDSM_ERR_DEVICE;
    else rc = hdsm_swarm_import_audit(swarm, d.audit.on ? 1 : 0, d.audit.sep_warn, rep.data());
  }
  return rc ? fail(rc, "state download failed") : HDSM_OK;
}

// ---- the phases of hdsm_dswarm_round, in the order of the header comment; every one issues on st and returns at its first error ----
#define PHASE_MARK(k) \
  do {                \
    if (d.phase_timing) HIP_TRY(hipEventRecord(d.ev[k].get(), st)); \
  } while (0)

// the path step (UpdatePath, AC:261-454) at the start of the round, before the corridor: every agent in rounds of the period,
// else the agents whose goal changed; no launch when nobody is due
int path_step(DSwarm& d, hipStream_t st) {
  PathStep& p = d.path;
  const bool all = p.period > 0 && p.round % p.period == 0;
  int n_plan = all ? d.n_fly() : p.n_due;
  if (!all && d.script.n > 0) {  // (the list of the due agents ascends: the flown ones come first)
    n_plan = 0;
    for (int k = 0; k < d.n_fly(); ++k) n_plan += p.due[(size_t)k] != 0;
  }
  p.timed.valid = false;
  if (n_plan > 0) {
    if (d.phase_timing) HIP_TRY(p.timed.record_start(st));
    if (p.dmp)
      hipLaunchKernelGGL(k_dmp, dim3((unsigned)n_plan), dim3(hdsm_path::THREADS), 0, st, d.c, all ? nullptr : p.d_due.get(), d.d_agents.get(),
                         p.d_goals.get(), p.d_cnt.get(), p.dmp_rn, p.d_dmp_rows.get());
    else
      hipLaunchKernelGGL(k_path, dim3((unsigned)n_plan), dim3(hdsm_path::THREADS), 0, st, d.c, all ? nullptr : p.d_due.get(), d.d_agents.get(),
                         p.d_goals.get(), p.d_cnt.get());
    HIP_TRY(hipGetLastError());
    if (d.phase_timing) HIP_TRY(p.timed.record_stop(st));
    ++p.launches;
  }
  p.n_due = 0;
  std::fill(p.due.begin(), p.due.end(), (uint8_t)0);
  ++p.round;
  return HDSM_OK;
}

// k_corridor, k_vel_cap, the reference, k_keep_free and the solve (marks 0 to 4)
int corridor_to_solve(DSwarm& d, hipStream_t st) {
  const int n = d.n_fly(), G = d.per * d.world;
  PHASE_MARK(0);
  if (n == 0) {
    for (int k = 1; k <= 4; ++k) PHASE_MARK(k);
    return HDSM_OK;
  }
  hipLaunchKernelGGL(k_corridor, dim3((unsigned)n), dim3(64), d.c.has_world ? hdsm_cd::wave_lds_bytes(hdsm_cd::wave_map_radius(d.c.n_it_decomp)) : 0, st, d.c,
                     n, d.d_agents.get(), d.d_path.get(), d.d_npath.get(), d.d_id.get(), d.d_state.get(), d.d_npoly.get(), d.d_nrows.get(), d.d_A.get(),
                     d.d_b.get(), d.d_cache.get());
  HIP_TRY(hipGetLastError());
  PHASE_MARK(1);
  if (d.c.has_world) {
    hipLaunchKernelGGL(k_vel_cap, dim3((unsigned)n), dim3(64), 0, st, d.c, d.rcfg, n, d.d_agents.get(), d.d_path.get(), d.d_npath.get(), d.d_cap.get());
    HIP_TRY(hipGetLastError());
  }
  PHASE_MARK(2);
  // Link faults: the OTHER agents are read from the view k_deliver keeps (seen / seen_has, advanced by shift), every agent's own plan
  // from the plans buffer, which stays the truth. The handle borrows the three arrays for the two launches of this round only.
  const Links& lk = d.links;
  const double* const plans = lk.on ? lk.d_seen.get() : d.d_plans.get();
  const uint8_t* const has = lk.on ? lk.d_seen_has.get() : d.d_has.get();
  struct Borrow {
    void* solver;
    bool on;
    ~Borrow() {
      if (on) (void)hdsm_set_plan_shift_device(solver, nullptr), (void)hdsm_set_own_plans_device(solver, nullptr, nullptr);
    }
  } borrow{d.solver, lk.on};
  if (lk.on) {
    int lrc = hdsm_set_plan_shift_device(d.solver, lk.d_shift.get());
    if (lrc == HDSM_OK) lrc = hdsm_set_own_plans_device(d.solver, d.d_plans.get(), d.d_has.get());
    if (lrc) return fail(lrc, std::string("link faults: ") + hdsm_last_error());
  }
  int rc = hdsm_reference_device(d.solver, &d.rcfg, n, G, d.d_id.get(), d.d_path.get(), d.d_npath.get(), PTS, d.c.has_world ? d.d_cap.get() : nullptr,
                                 plans, has, d.d_ref_full.get(), d.d_ref.get(), d.d_pv.get(), st);
  if (rc) return fail(rc, std::string("hdsm_reference_device: ") + hdsm_last_error());
  PHASE_MARK(3);
  if (d.c.has_world) {
    hipLaunchKernelGGL(k_keep_free, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d.c, n, d.d_agents.get(), d.d_ref_full.get(), d.d_ref.get(),
                       d.d_pv.get());
    HIP_TRY(hipGetLastError());
  }
  PHASE_MARK(4);
  rc = hdsm_replan_device(d.solver, n, G, d.d_id.get(), d.d_state.get(), d.d_ref.get(), d.d_npoly.get(), d.d_nrows.get(), d.d_A.get(), d.d_b.get(),
                          plans, has, d.d_traj.get(), d.d_ctrl.get(), d.d_used.get(), d.d_status.get(), d.d_obj.get(), st);
  if (rc) return fail(rc, std::string("hdsm_replan_device: ") + hdsm_last_error());
  return HDSM_OK;
}

// k_commit (mark 5, and mark 6 unless the rank is a local one). One rank without a local communicator: the solve of this round is
// behind us on the stream, so the records go straight into the plans buffer — slot k = agent k — and the flags with them; several
// ranks, and every local rank (`local`: its communicator, else NULL): into the send buffer of the ONE all-gather. A local rank's
// k_commit waits until every rank has gathered the round before — until then its send buffer may still be read — and is followed by
// the rank's "published" event; its mark 6 stands in front of the gather (exchange).
int commit(DSwarm& d, void* local, hipStream_t st) {
  PHASE_MARK(5);
  const bool direct = d.world == 1 && local == nullptr;
  if (local)
    if (int rc = hdsm_internal_local_commit_gate(local, st)) return fail(rc, std::string("local ranks: ") + hdsm_last_error());
  const int n_fly = d.n_fly();
  hipLaunchKernelGGL(k_commit, dim3((unsigned)(d.per > 0 ? d.per : 1)), dim3(64), 0, st, d.c, n_fly, d.per, d.d_agents.get(), d.d_traj.get(),
                     d.d_ctrl.get(), d.d_used.get(), d.d_status.get(), direct ? d.d_plans.get() : d.d_local.get(), d.d_fails.get(),
                     direct ? d.d_has.get() : nullptr, d.d_ref_full.get(), d.d_pv.get());
  HIP_TRY(hipGetLastError());
  if (Track& t = d.track; t.on) {  // the flown agents fly something else than they planned (inside phase [5]; the records above stay the plans)
    if (n_fly > 0) {
      HIP_TRY(hdsm_track::launch(hdsm_track::Launch{n_fly, d.c.step_plan, t.q, (double)d.c.step_plan * d.prm.dt, t.model, d.d_agents.get(), t.d_rec.get(),
                                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
                                 st));
      ++t.model_launches;
    }
    ++t.q;
  }
  if (Script& s = d.script; s.n > 0) {  // the scripted tail, over the slots k_commit has just padded (and inside its phase [5])
    const size_t rec = (size_t)(d.c.N + 1) * 9;
    HIP_TRY(hdsm_script::launch(hdsm_script::Round{s.n, s.n_knots, d.c.N, d.c.step_plan, s.predict, s.round, d.prm.dt, s.d_knots.get(),
                                                   (direct ? d.d_plans.get() : d.d_local.get()) + (size_t)n_fly * rec,
                                                   direct ? d.d_has.get() + n_fly : nullptr, d.d_status.get() + n_fly, d.d_agents.get() + n_fly},
                                st));
    ++s.round, ++s.launches;
  }
  if (local) {
    if (int rc = hdsm_internal_local_published(local, st)) return fail(rc, std::string("local ranks: ") + hdsm_last_error());
  } else {
    PHASE_MARK(6);
  }
  return HDSM_OK;
}

// the exchange (up to mark 7): ONE RCCL all-gather, nothing on a single rank, or the gather of a local rank (k_gather_local: it waits
// for every rank's "published", and mark 6 is recorded behind those waits, so that [6] of the phase timing is the gather itself)
int exchange(DSwarm& d, void* comm, void* local, hipStream_t st) {
  if (local) {
    const int rc = hdsm_internal_local_gather(local, d.d_plans.get(), d.d_has.get(), st, d.phase_timing ? d.ev[6].get() : nullptr);
    if (rc) return fail(rc, std::string("local ranks: ") + hdsm_last_error());
  } else if (d.world > 1) {
    const int rc = hdsm_exchange_device(comm, d.per, d.d_local.get(), d.d_plans.get(), d.d_has.get(), st);
    if (rc) return fail(rc, std::string("hdsm_exchange_device: ") + hdsm_last_error());
  }
  PHASE_MARK(7);
  return HDSM_OK;
}
#undef PHASE_MARK

// link faults: the records the exchange has just left in the plans buffer meet their fates (k_deliver; only while links are on)
hdsm_link::Round link_round(const DSwarm& d) {
  const Links& l = d.links;
  return hdsm_link::Round{d.per * d.world, d.n_rob, d.c.N, d.c.step_plan, l.n_rounds, l.D, l.time_aware, l.round, l.d_fate.get(), d.d_plans.get(),
                          l.d_ring.get(), l.d_seen.get(), l.d_seen_has.get(), l.d_seen_round.get(), l.d_shift.get(), l.d_cnt.get()};
}
int deliver(DSwarm& d, hipStream_t st) {
  Links& l = d.links;
  const int G = d.per * d.world;
  if (!l.on || G == 0) return HDSM_OK;
  hipLaunchKernelGGL(k_deliver, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, st, link_round(d));
  HIP_TRY(hipGetLastError());
  ++l.round;
  return HDSM_OK;
}

// the flight audit and the history row, on this round's records of all agents (only when one of them is on)
int audit_and_history(DSwarm& d, hipStream_t st) {
  Audit& a = d.audit;
  History& h = d.hist;
  const int n = d.n_local;
  a.timed.valid = false;
  if (h.cap > 0 && h.n == h.cap) ++h.dropped;
  const bool hist = h.cap > 0 && h.n < h.cap;
  if ((a.on || hist) && n > 0) {
    if (d.phase_timing) HIP_TRY(a.timed.record_start(st));
    hdsm_audit::World wd{};
    wd.world = d.c.has_world ? d.d_world.get() : nullptr, wd.voxel_size = d.c.voxel_size;
    for (int k = 0; k < 3; ++k) wd.wdim[k] = d.c.wdim[k], wd.worigin[k] = d.c.worigin[k];
    HIP_TRY(hdsm_audit::launch(a.buf, a.on, d.d_plans.get(), d.d_has.get(), d.d_range.get(), d.c.N, d.first,
                               hdsm_audit::weights(d.prm.drone_radius, d.prm.drone_z_offset), wd, a.d_report.get(), a.sep_warn * a.sep_warn, &d.d_agents.get()[0].state_curr[0], sizeof(AgentS),
                               hist ? h.d_rows.get() + (size_t)h.n * n * 9 : nullptr, st));
    if (d.phase_timing) HIP_TRY(a.timed.record_stop(st));
    if (a.on) ++a.rounds;
  }
  if (hist) ++h.n;
  h.last = hist;
  return HDSM_OK;
}

// The round is issued on ONE stream and says so to the solver handle: the pre-pass of the solve then rides on the reference kernel
// (hdsm_api.hip, `packed`). At its end it names the point a later call on another stream has to wait for; the handle records its
// "done" event only when such a call arrives (hdsm_entry.h) — a record is a barrier packet, 5-6 us of idle queue in front of the next kernel.
struct DoneOnce {
  void* solver;
  hipStream_t st;
  DoneOnce(void* s, hipStream_t q) : solver(s), st(q) { (void)hdsm_internal_defer_done(solver, 1); }
  ~DoneOnce() {
    (void)hdsm_internal_defer_done(solver, 0);
    (void)hdsm_internal_record_done(solver, st);
  }
};

// The two halves of a round. hdsm_dswarm_round issues one behind the other; hdsm_dswarm_round_ranks the front of every rank, then the
// back of every rank (no rank can gather what another has not been asked to publish). `local`: the rank's local communicator or NULL.
int round_front(DSwarm& d, void* local, hipStream_t st) {
  if (int rc = path_step(d, st)) return rc;
  if (int rc = corridor_to_solve(d, st)) return rc;
  return commit(d, local, st);
}
int round_back(DSwarm& d, void* comm, void* local, hipStream_t st) {
  if (int rc = exchange(d, comm, local, st)) return rc;
  if (int rc = deliver(d, st)) return rc;
  if (int rc = audit_and_history(d, st)) return rc;
  if (d.phase_timing) d.phase_valid = true;
  ++d.rounds;
  return HDSM_OK;
}

// the communicator must be the one this shard was cut for: its rank's block starts at first
int check_comm(const DSwarm& d, void* comm) {
  int32_t crank = -1, cworld = -1;
  if (hdsm_comm_info(comm, &crank, &cworld) != HDSM_OK) return fail(HDSM_ERR_COMM, std::string("hdsm_comm_info: ") + hdsm_last_error());
  const bool empty_tail = d.n_local == 0 && d.first == d.n_rob;  // (any rank behind the last agent)
  if (cworld != d.world || (d.per > 0 && (empty_tail ? (int64_t)crank * d.per < d.n_rob : crank != d.first / d.per)))
    return fail(HDSM_ERR_BAD_ARG, "communicator rank / size do not match the shard (first_id / per, world_size)");
  return HDSM_OK;
}

}  // namespace

extern "C" {

const char* hdsm_dswarm_last_error(void) { return g_err.c_str(); }

// The flight per group (one record for the whole swarm without a partition): k_group_report over the agents' states, the last
// statuses and — once the audit has been on — the flight records. Launched here and nowhere else: a round never pays for it.
int hdsm_dswarm_group_report(void* dswarm, hdsm_group_report* out) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  const int ng = (int)d->group_start.size() - 1;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!d->d_gstart) {
    HIP_TRY(d->d_gstart.alloc(d->group_start.size()));
    HIP_TRY(hipMemcpy(d->d_gstart.get(), d->group_start.data(), d->group_start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(d->d_greport.alloc((size_t)ng));
  }
  hipLaunchKernelGGL(k_group_report, dim3((unsigned)ng), dim3(64), 0, nullptr, d->first, d->n_local, d->d_gstart.get(), d->d_agents.get(), d->d_status.get(),
                     d->audit.ever ? d->audit.d_report.get() : nullptr, d->d_greport.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d->d_greport.get(), (size_t)ng * sizeof(hdsm_group_report), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// Where a round of the device-resident loop goes, measured with HIP events on the round's own stream: the records sit between the
// launches of hdsm_dswarm_round — [0] k_corridor, [1] k_vel_cap, [2] hdsm_reference_device (pack + reference), [3] k_keep_free,
// [4] hdsm_replan_device (pre-pass, solver kernels, merge), [5] k_commit, [6] the exchange. hdsm_dswarm_last_phase_ms synchronises
// with the last timed round and returns the seven durations in milliseconds (a phase the round did not launch: ~0).
int hdsm_dswarm_set_phase_timing(void* dswarm, int32_t on) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  HIP_TRY(hipSetDevice(d->device));
  if (on)
    if (int rc = timing_events(d)) return rc;
  d->phase_timing = on != 0, d->phase_valid = false, d->path.timed.valid = false, d->audit.timed.valid = false;
  return HDSM_OK;
}

// The polyhedron cache of the device corridor (k_corridor, PolyCache), summed over the shard's agents since hdsm_dswarm_create:
// out[0] polyhedra asked for, out[1] formed from a cached structure recorded in the same local grid, out[2] formed from one recorded in
// ANOTHER grid at the same height (the interior rule), out[3] = 1 if the cache is on (HDSM_POLY_CACHE, a world is set), else 0.
int hdsm_dswarm_cache_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!d->d_cache || d->n_local == 0) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  out[3] = 1;
  // (only the four counters of every entry travel: one strided 2-D copy)
  std::vector<int32_t> cnt((size_t)d->n_local * 4);
  HIP_TRY(hipMemcpy2D(cnt.data(), 16, reinterpret_cast<const char*>(d->d_cache.get()) + offsetof(PolyCache, asked), sizeof(PolyCache), 16,
                      (size_t)d->n_local, hipMemcpyDeviceToHost));
  for (int k = 0; k < d->n_local; ++k) out[0] += cnt[4 * (size_t)k], out[1] += cnt[4 * (size_t)k + 1], out[2] += cnt[4 * (size_t)k + 2];
  return HDSM_OK;
}

int hdsm_dswarm_last_phase_ms(void* dswarm, float ms[7]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !ms) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->phase_valid) return fail(HDSM_ERR_BAD_ARG, "no round has run with hdsm_dswarm_set_phase_timing on");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipEventSynchronize(d->ev[7].get()));
  for (int k = 0; k < 7; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], d->ev[k].get(), d->ev[k + 1].get()));
  return HDSM_OK;
}

// The path step of the last timed round that launched k_path, in milliseconds (0 if it planned no agent): kept out of
// hdsm_dswarm_last_phase_ms, whose [0] k_corridor starts after it.
int hdsm_dswarm_last_path_ms(void* dswarm, float* ms) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !ms) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->phase_valid) return fail(HDSM_ERR_BAD_ARG, "no round has run with hdsm_dswarm_set_phase_timing on");
  *ms = 0.0f;
  if (!d->path.timed.valid) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(d->path.timed.ms(ms));
  return HDSM_OK;
}

// GoalCallback (AC:2380-2388) for the shard: goals [n_local][3]; the agents whose goal changed plan a new path at the start of
// the next round (k_path). Synchronises the device.
int hdsm_dswarm_set_goals(void* dswarm, const double* goals) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (!goals && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (d->n_local == 0) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  PathStep& p = d->path;
  for (int k = 0; k < d->n_local; ++k) {
    double* g = &p.goals[3 * (size_t)k];
    const double* ng = goals + 3 * (size_t)k;
    if (g[0] == ng[0] && g[1] == ng[1] && g[2] == ng[2]) continue;
    g[0] = ng[0], g[1] = ng[1], g[2] = ng[2];
    p.due[k] = 1;
  }
  std::vector<int32_t> idx;
  for (int k = 0; k < d->n_local; ++k)
    if (p.due[k]) idx.push_back(k);
  p.n_due = (int)idx.size();
  HIP_TRY(hipMemcpy(p.d_goals.get(), p.goals.data(), p.goals.size() * sizeof(double), hipMemcpyHostToDevice));
  if (p.n_due) HIP_TRY(hipMemcpy(p.d_due.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return HDSM_OK;
}

// out[0] agents planned by k_path since hdsm_dswarm_create, out[1] of them without a new path, out[2] launches of k_path.
// Synchronises the device.
int hdsm_dswarm_path_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, d->path.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost));
  out[0] = (int64_t)cnt[0], out[1] = (int64_t)cnt[1], out[2] = d->path.launches;
  return HDSM_OK;
}

int hdsm_dswarm_create(void* swarm, void* solver, int32_t device, int32_t world_size, void** dswarm) {
  if (!swarm || !solver || !dswarm || world_size < 1) return fail(HDSM_ERR_BAD_ARG, "null argument");
  *dswarm = nullptr;
  std::unique_ptr<DSwarm> d(new (std::nothrow) DSwarm);
  if (!d) return fail(HDSM_ERR_DEVICE, "out of host memory");
  d->solver = solver, d->device = device, d->world = world_size;
  const int8_t* hworld = nullptr;
  int32_t wdim[3] = {0, 0, 0};
  double worigin[3] = {0, 0, 0};
  if (int rc = hdsm_swarm_export_state(swarm, nullptr, &d->n_local, &d->n_rob, &d->first, &d->prm, &d->cfg, &hworld, wdim, worigin))
    return fail(rc, "hdsm_swarm_export_state");
  d->per = (d->n_rob + world_size - 1) / world_size;
  if (d->n_local > d->per) return fail(HDSM_ERR_BAD_ARG, "the shard is larger than ceil(n_rob / world_size)");
  // Layout contract of the device loop (hdsm_swarm.h): the plans buffer holds agent a's record at slot a — the all-gather puts
  // rank r's block at r * per, a single rank copies its block to slot 0 — and the solver finds an agent's OWN plan (and skips
  // its own record in the sweeps) by agent id. So the shard must be the block of a rank of the ceil(n_rob / world_size) split.
  // (An EMPTY trailing shard — n_rob = 5 on 4 ranks leaves rank 3 with first_id = n_rob and no agent, what swarm.shard_range
  // produces — is a valid block; its rank comes from the communicator, not from first_id / per.)
  const bool empty_tail = d->n_local == 0 && d->first == d->n_rob;
  if (d->per > 0 && !empty_tail &&
      (d->first % d->per != 0 || (d->n_local < d->per && d->first + d->n_local != d->n_rob) || (world_size == 1 && d->first != 0)))
    return fail(HDSM_ERR_BAD_ARG, "the shard is not a block of the ceil(n_rob / world_size) split: first_id must be rank * per, a short "
                                  "shard must be the last one (and first_id 0 with world_size 1)");
  d->rcfg = {d->cfg.path_vel_min, d->cfg.path_vel_max, d->cfg.sens_dist, d->cfg.sens_pot, d->cfg.sens_other_agents, d->cfg.path_vel_dec};
  Cfg& c = d->c;
  c.N = d->prm.n_hor, c.P = d->prm.poly_hor, c.RS = d->prm.max_rows_static, c.step_plan = d->cfg.step_plan;
  c.n_it_decomp = d->cfg.n_it_decomp, c.use_cvx_new = d->cfg.use_cvx_new, c.has_world = hworld ? 1 : 0;
  c.voxel_size = d->cfg.voxel_size, c.grid_z_min = d->cfg.grid_z_min, c.thresh_dist = d->cfg.thresh_dist;
  c.fast_walk = 1;
  if (const char* e = std::getenv("HDSM_FAST_WALK")) {  // development switch (A/B of the walk shortcut): "0" or "1", anything else is ignored
    if ((e[0] == '0' || e[0] == '1') && e[1] == 0) c.fast_walk = e[0] == '1';
  }
  for (int k = 0; k < 3; ++k) c.grid_range[k] = d->cfg.grid_range[k], c.wdim[k] = wdim[k], c.worigin[k] = worigin[k];
  if (hipSetDevice(device) != hipSuccess) return fail(HDSM_ERR_NO_DEVICE, "hipSetDevice failed");
  const hipError_t e = alloc_round_buffers(d.get(), hworld);
  if (e != hipSuccess) return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_create: ") + hipGetErrorString(e));
  if (int rc = take_over(*d, swarm, hworld)) return rc;
  *dswarm = d.release();
  return HDSM_OK;
}

void hdsm_dswarm_destroy(void* dswarm) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return;
  (void)hipSetDevice(d->device);
  (void)hipDeviceSynchronize();
  delete d;
}

int hdsm_dswarm_round(void* dswarm, void* comm, void* hip_stream) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (d->world > 1 && !comm) return fail(HDSM_ERR_BAD_ARG, "a sharded swarm needs a communicator");
  if (comm) {
    if (hdsm_internal_comm_kind(comm, nullptr) == 1) return fail(HDSM_ERR_BAD_ARG, HDSM_LOCAL_COMM_REFUSED);
    if (int rc = check_comm(*d, comm)) return rc;
  }
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DoneOnce done_once(d->solver, st);
  if (int rc = round_front(*d, nullptr, st)) return rc;
  return round_back(*d, comm, nullptr, st);
}

int hdsm_dswarm_round_ranks(int32_t world, void* const* dswarms, void* const* comms, void* const* hip_streams) {
  if (world < 1 || !dswarms || !comms) return fail(HDSM_ERR_BAD_ARG, "bad hdsm_dswarm_round_ranks argument");
  for (int r = 0; r < world; ++r)
    if (!dswarms[r] || !comms[r]) return fail(HDSM_ERR_BAD_ARG, "null dswarm or communicator of rank " + std::to_string(r));
  const DSwarm* d0 = static_cast<const DSwarm*>(dswarms[0]);
  if (int rc = hdsm_internal_local_check(world, comms, (d0->c.N + 1) * 9)) return fail(rc, std::string("hdsm_dswarm_round_ranks: ") + hdsm_last_error());
  std::vector<const double*> send((size_t)world);
  for (int r = 0; r < world; ++r) {
    const DSwarm* d = static_cast<const DSwarm*>(dswarms[r]);
    for (int q = 0; q < r; ++q)
      if (dswarms[q] == dswarms[r]) return fail(HDSM_ERR_BAD_ARG, "the dswarm of rank " + std::to_string(q) + " is given again for rank " + std::to_string(r));
    // (the gather of every rank copies per * rec doubles out of every send buffer: one n_rob, one n_hor)
    if (d->n_rob != d0->n_rob || d->c.N != d0->c.N) return fail(HDSM_ERR_BAD_ARG, "the shards of ranks 0 and " + std::to_string(r) + " differ in n_rob or n_hor");
    if (int rc = check_comm(*d, comms[r])) return rc;
    int32_t cdev = -1;
    (void)hdsm_internal_comm_kind(comms[r], &cdev);
    if (cdev != d->device) return fail(HDSM_ERR_BAD_ARG, "the dswarm of rank " + std::to_string(r) + " is not on the device of its communicator's handle");
    send[(size_t)r] = d->d_local.get();
  }
  if (int rc = hdsm_internal_local_bind(world, comms, send.data(), d0->per)) return fail(rc, std::string("hdsm_dswarm_round_ranks: ") + hdsm_last_error());
  // every "published" is recorded (front) before a gather waits for it (back); every "gathered" before the next round's k_commit does
  for (int r = 0; r < world; ++r) {
    DSwarm* d = static_cast<DSwarm*>(dswarms[r]);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = static_cast<hipStream_t>(hip_streams ? hip_streams[r] : nullptr);
    DoneOnce done_once(d->solver, st);
    if (int rc = round_front(*d, comms[r], st)) return rc;
  }
  for (int r = 0; r < world; ++r) {
    DSwarm* d = static_cast<DSwarm*>(dswarms[r]);
    HIP_TRY(hipSetDevice(d->device));
    if (int rc = round_back(*d, comms[r], comms[r], static_cast<hipStream_t>(hip_streams ? hip_streams[r] : nullptr))) return rc;
  }
  return HDSM_OK;
}

// Link faults (include/hdsm_swarm.h). The call starts a new link history: the view is the plans buffer as it stands (every slot
// delivered on time, held round -1, shift 0), the counters are zero, link round 0 is the next round.
int hdsm_dswarm_set_links(void* dswarm, int32_t n_rounds, const int8_t* fate, int32_t time_aware) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (n_rounds < 0) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_links: negative n_rounds");
  Links& l = d->links;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (n_rounds == 0 || fate == nullptr) {
    l.on = false;
    return HDSM_OK;
  }
  const int D = hdsm_link::table_max_delay(n_rounds, d->n_rob, fate);
  if (D < 0) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_links: a delay above HDSM_LINK_MAX_DELAY");
  const size_t G = (size_t)d->per * d->world, rec = (size_t)(d->c.N + 1) * 9, cells = (size_t)n_rounds * (size_t)d->n_rob;
  l.on = false;
  if (!l.ready()) {  // the first call: everything but the table, whose size is the caller's
    hdsm_mem::FirstError ok;
    ok(l.d_ring.alloc_zeroed((size_t)(hdsm_link::MAX_DELAY + 1) * G * rec)), ok(l.d_seen.alloc_zeroed(G * rec)), ok(l.d_seen_has.alloc_zeroed(G));
    ok(l.d_seen_round.alloc(G)), ok(l.d_shift.alloc(G)), ok(l.d_cnt.alloc(G * hdsm_link::COUNTERS));
    if (!ok.ok()) {
      l.d_cnt.reset();
      return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_set_links: ") + hipGetErrorString(ok.e));
    }
  }
  HIP_TRY(l.d_fate.ensure(cells, nullptr));
  if (cells) HIP_TRY(hipMemcpy(l.d_fate.get(), fate, cells, hipMemcpyHostToDevice));
  if (G) {
    HIP_TRY(hipMemcpy(l.d_seen.get(), d->d_plans.get(), G * rec * 8, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(l.d_seen_has.get(), d->d_has.get(), G, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemset(l.d_seen_round.get(), 0xff, G * sizeof(int32_t)));  // -1
    HIP_TRY(hipMemset(l.d_shift.get(), 0, G * sizeof(int32_t)));
    HIP_TRY(hipMemset(l.d_cnt.get(), 0, G * hdsm_link::COUNTERS * sizeof(int32_t)));
  }
  l.n_rounds = n_rounds, l.D = D, l.time_aware = time_aware != 0, l.round = 0, l.on = true;
  return HDSM_OK;
}

// Scripted agents (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_script(void* dswarm, int32_t n_script, int32_t n_knots, const double* knots, int32_t predict) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  Script& s = d->script;
  if (n_script < s.n) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: n_script may stay or grow (a scripted agent has no planner state to resume from)");
  if (n_script > d->n_local) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: more scripted agents than the shard has");
  if (predict != 0 && predict != 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: predict is 0 or 1");
  if (!hdsm_script::tracks_valid(n_script, n_knots, knots))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: 1 .. 256 knots per track, every entry finite, times strictly increasing");
  if (n_script == 0) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!s.d_knots) HIP_TRY(s.d_knots.alloc((size_t)d->n_local * hdsm_script::MAX_KNOTS * 4));
  HIP_TRY(hipMemcpy(s.d_knots.get(), knots, (size_t)n_script * n_knots * 4 * sizeof(double), hipMemcpyHostToDevice));
  // a scripted agent's goal is its last knot, and it plans no path: the flown agents that are due stay due
  PathStep& p = d->path;
  const int n_fly = d->n_local - n_script;
  std::vector<int32_t> idx;
  for (int k = 0; k < d->n_local; ++k) {
    if (k >= n_fly) {
      const double* last = knots + ((size_t)(k - n_fly) * n_knots + (n_knots - 1)) * 4;
      for (int q = 0; q < 3; ++q) p.goals[3 * (size_t)k + q] = last[1 + q];
      p.due[(size_t)k] = 0;
    }
    if (p.due[(size_t)k]) idx.push_back(k);
  }
  p.n_due = (int)idx.size();
  HIP_TRY(hipMemcpy(p.d_goals.get(), p.goals.data(), p.goals.size() * sizeof(double), hipMemcpyHostToDevice));
  if (p.n_due) HIP_TRY(hipMemcpy(p.d_due.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  s.n = n_script, s.n_knots = n_knots, s.predict = predict, s.round = 0;
  return HDSM_OK;
}

int hdsm_dswarm_script_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->script.round, out[1] = d->script.n, out[2] = d->script.launches;
  return HDSM_OK;
}

// Imperfect tracking (include/hdsm_swarm.h). Every refusal comes before anything is touched.
namespace {
// the records, allocated by the first call that needs them (the caller has set the device)
int track_records_ready(DSwarm* d) {
  if (!d->track.d_rec) {
    HIP_TRY(d->track.d_rec.alloc_zeroed((size_t)d->n_local));
    HIP_TRY(hipDeviceSynchronize());  // (the fill is done before a kernel of any stream books into them)
  }
  return HDSM_OK;
}
// a state from outside into the flown agents: k_track's external form over device arrays, on st
int track_external(DSwarm* d, const double* d_states, const uint8_t* d_mask, hipStream_t st) {
  Track& t = d->track;
  const History& h = d->hist;
  const int n_fly = d->n_fly();
  if (n_fly > 0) {
    // the state measured behind a round IS the state after that round: the row the round left in the history takes it too
    double* const row = h.last && h.n > 0 ? h.d_rows.get() + (size_t)(h.n - 1) * d->n_local * 9 : nullptr;
    HIP_TRY(hdsm_track::launch(hdsm_track::Launch{n_fly, d->c.step_plan, 0, 0.0, hdsm_tracking{}, d->d_agents.get(), t.d_rec.get(), d_states, d_mask, nullptr,
                                                  nullptr, nullptr, nullptr, row},
                               st));
    ++t.external_launches;
  }
  return HDSM_OK;
}
}  // namespace

int hdsm_dswarm_set_tracking(void* dswarm, const hdsm_tracking* m) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (m && !hdsm_track::model_valid(m))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_tracking: every entry of the model finite, gust and jitter not negative");
  Track& t = d->track;
  if (!m && !t.on) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (m) {
    if (int rc = track_records_ready(d)) return rc;
    t.model = *m, t.q = 0;
  }
  t.on = m != nullptr;
  return HDSM_OK;
}

int hdsm_dswarm_set_states(void* dswarm, const double* states, const uint8_t* mask) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (!states && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_states: null argument");
  if (d->n_local == 0) return HDSM_OK;
  Track& t = d->track;
  const size_t n = (size_t)d->n_local;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = track_records_ready(d)) return rc;
  if (!t.d_stage) HIP_TRY(t.d_stage.alloc(n * 9));
  if (mask && !t.d_stage_mask) HIP_TRY(t.d_stage_mask.alloc(n));
  HIP_TRY(hipMemcpy(t.d_stage.get(), states, n * 9 * sizeof(double), hipMemcpyHostToDevice));
  if (mask) HIP_TRY(hipMemcpy(t.d_stage_mask.get(), mask, n, hipMemcpyHostToDevice));
  if (int rc = track_external(d, t.d_stage.get(), mask ? t.d_stage_mask.get() : nullptr, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

int hdsm_dswarm_set_states_device(void* dswarm, const double* d_states, const uint8_t* d_mask, void* hip_stream) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (!d_states && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_states_device: null argument");
  if (d->n_local == 0) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  if (int rc = track_records_ready(d)) return rc;
  return track_external(d, d_states, d_mask, static_cast<hipStream_t>(hip_stream));
}

int hdsm_dswarm_track_records(void* dswarm, hdsm_track_record* out) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (!out && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_track_records: null argument");
  if (d->n_local == 0) return HDSM_OK;
  if (!d->track.d_rec) {
    for (int k = 0; k < d->n_local; ++k) out[k] = hdsm_track_record{};
    return HDSM_OK;
  }
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d->track.d_rec.get(), (size_t)d->n_local * sizeof(hdsm_track_record), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_track_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->track.q, out[1] = d->track.model_launches, out[2] = d->track.external_launches;
  return HDSM_OK;
}

int hdsm_dswarm_plans_device(void* dswarm, void** d_plans, void** d_has) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !d_plans || !d_has) return fail(HDSM_ERR_BAD_ARG, "null argument");
  *d_plans = d->d_plans.get(), *d_has = d->d_has.get();
  return HDSM_OK;
}

int hdsm_dswarm_link_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!d->links.ready()) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = (size_t)d->per * d->world, have = (size_t)d->n_rob < G ? (size_t)d->n_rob : G;  // (the padded tail publishes nothing)
  std::vector<int32_t> cnt(have * hdsm_link::COUNTERS + 1);
  if (have) HIP_TRY(hipMemcpy(cnt.data(), d->links.d_cnt.get(), have * hdsm_link::COUNTERS * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < have; ++k) {
    const int32_t* c = &cnt[k * hdsm_link::COUNTERS];
    out[1] += c[0], out[2] += c[1];
    out[3] = c[2] > out[3] ? c[2] : out[3], out[0] = c[3] > out[0] ? c[3] : out[0];
  }
  return HDSM_OK;
}

int hdsm_dswarm_download_seen(void* dswarm, double* seen_raw, uint8_t* seen_has, int32_t* seen_round, int32_t* shift) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (!d->links.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_download_seen: no hdsm_dswarm_set_links yet");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const Links& l = d->links;
  const size_t G = (size_t)d->per * d->world, rec = (size_t)(d->c.N + 1) * 9;
  if (G == 0) return HDSM_OK;
  if (seen_raw) HIP_TRY(hipMemcpy(seen_raw, l.d_seen.get(), G * rec * 8, hipMemcpyDeviceToHost));
  if (seen_has) HIP_TRY(hipMemcpy(seen_has, l.d_seen_has.get(), G, hipMemcpyDeviceToHost));
  if (seen_round) HIP_TRY(hipMemcpy(seen_round, l.d_seen_round.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (shift) HIP_TRY(hipMemcpy(shift, l.d_shift.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_download_raw(void* dswarm, double* plans_all_raw, double* send_raw) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t L = (size_t)d->per, G = (size_t)d->per * d->world, rec = (size_t)(d->c.N + 1) * 9;
  if (plans_all_raw && G) HIP_TRY(hipMemcpy(plans_all_raw, d->d_plans.get(), G * rec * 8, hipMemcpyDeviceToHost));
  if (send_raw && L) HIP_TRY(hipMemcpy(send_raw, d->d_local.get(), L * rec * 8, hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_upload_plans(void* dswarm, const double* plans_all, const uint8_t* has_plan) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !plans_all || !has_plan) return fail(HDSM_ERR_BAD_ARG, "null argument");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = (size_t)d->per * d->world, rec = (size_t)(d->c.N + 1) * 9, have = (size_t)d->n_rob < G ? (size_t)d->n_rob : G;
  HIP_TRY(hipMemset(d->d_has.get(), 0, G));
  HIP_TRY(hipMemcpy(d->d_plans.get(), plans_all, have * rec * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d->d_has.get(), has_plan, have, hipMemcpyHostToDevice));
  return HDSM_OK;
}

int hdsm_dswarm_download(void* dswarm, void* swarm, double* plans_all, uint8_t* has_plan, int32_t* status, int32_t* failed_total) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = (size_t)d->n_local, G = (size_t)d->per * d->world, rec = (size_t)(d->c.N + 1) * 9;
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

// ---- the flight audit and the state history of the device loop (audit_kernels.hip) ----
int hdsm_dswarm_set_audit(void* dswarm, int32_t on, double sep_warn) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (!(sep_warn > 0)) return fail(HDSM_ERR_BAD_ARG, "sep_warn must be positive");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  d->audit.on = on != 0, d->audit.sep_warn = sep_warn;
  if (on) {
    if (int rc = audit_setup(d, nullptr)) return rc;
    if (d->phase_timing)
      if (int rc = timing_events(d)) return rc;
  }
  return HDSM_OK;
}

int hdsm_dswarm_flight_report(void* dswarm, hdsm_flight_report* report) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (d->n_local && !report)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->audit.ever) return fail(HDSM_ERR_BAD_ARG, "the flight audit was never switched on");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (d->n_local) HIP_TRY(hipMemcpy(report, d->audit.d_report.get(), (size_t)d->n_local * sizeof(hdsm_flight_report), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_last_audit_round(void* dswarm, hdsm_audit_round* out) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || (d->n_local && !out)) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->audit.on || d->audit.rounds == 0) return fail(HDSM_ERR_BAD_ARG, "no round has been audited (hdsm_dswarm_set_audit)");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (d->n_local) HIP_TRY(hipMemcpy(out, d->audit.buf.d_round.get(), (size_t)d->n_local * sizeof(hdsm_audit_round), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// The audit's launches of the last timed round (pack, sweep, track; or the history write alone), in milliseconds; 0 when that round
// launched none or no round was timed. Kept out of hdsm_dswarm_last_phase_ms: the audit starts after its [6].
int hdsm_dswarm_last_audit_ms(void* dswarm, float* ms) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !ms) return fail(HDSM_ERR_BAD_ARG, "null argument");
  *ms = 0.0f;
  if (!d->audit.timed.valid) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(d->audit.timed.ms(ms));
  return HDSM_OK;
}

int hdsm_dswarm_set_history(void* dswarm, int32_t capacity_rounds) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || capacity_rounds < 0) return fail(HDSM_ERR_BAD_ARG, "bad argument");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  History& h = d->hist;
  h.d_rows.reset();
  h.cap = 0, h.n = h.dropped = h.delivered = 0, h.last = false;
  if (capacity_rounds > 0) {
    if (int rc = audit_setup(d, nullptr)) return rc;
    HIP_TRY(h.d_rows.alloc((size_t)capacity_rounds * d->n_local * 9 + 1));
    h.cap = capacity_rounds;
    if (d->phase_timing)
      if (int rc = timing_events(d)) return rc;
  }
  return HDSM_OK;
}

int hdsm_dswarm_download_history(void* dswarm, void* swarm, double* hist, int32_t max_rounds, int32_t* n_rounds, int32_t* dropped) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || max_rounds < 0 || (hist == nullptr && max_rounds > 0)) return fail(HDSM_ERR_BAD_ARG, "bad argument");
  History& h = d->hist;
  if (h.cap == 0) return fail(HDSM_ERR_BAD_ARG, "the history is off (hdsm_dswarm_set_history)");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t row = (size_t)d->n_local * 9;
  const int n_copy = h.n < max_rounds ? h.n : max_rounds;
  if (n_copy > 0 && row) HIP_TRY(hipMemcpy(hist, h.d_rows.get(), (size_t)n_copy * row * sizeof(double), hipMemcpyDeviceToHost));
  if (swarm && h.n > h.delivered) {  // every recorded round reaches the mirror's planner records once
    const int m = h.n - h.delivered;
    std::vector<double> rows((size_t)m * row);
    if (row) HIP_TRY(hipMemcpy(rows.data(), h.d_rows.get() + (size_t)h.delivered * row, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int rc = hdsm_swarm_append_history(swarm, m, rows.data());
    if (rc) return fail(rc, "hdsm_swarm_append_history");
    h.delivered = h.n;
  }
  if (n_rounds) *n_rounds = h.n;
  if (dropped) *dropped = h.dropped;
  return HDSM_OK;
}

// ---- map updates in flight (ABI 1.7; semantics in hdsm_swarm.h) ----
int hdsm_dswarm_update_world(void* dswarm, const int8_t* values, const int32_t lo[3], const int32_t bdim[3]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k <= 0) return k;
  if (!values) return fail(HDSM_ERR_BAD_ARG, "null values");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = stage_box(d, values, bdim)) return rc;
  if (int rc = put_box(d, d->edits.d_edit.get(), d->d_world.get(), lo, bdim, nullptr)) return rc;
  if (int rc = invalidate(d, lo, bdim, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  ++d->edits.updates, d->edits.voxels += (long long)bdim[0] * bdim[1] * bdim[2];
  return HDSM_OK;
}

int hdsm_dswarm_set_raw_world(void* dswarm, const hdsm_map_config* map_cfg, const int8_t* raw_full) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !map_cfg || !raw_full) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return fail(HDSM_ERR_BAD_ARG, "the dswarm has no world (hdsm_swarm_set_world before hdsm_dswarm_create)");
  const size_t vox = (size_t)d->c.wdim[0] * d->c.wdim[1] * d->c.wdim[2];
  for (size_t i = 0; i < vox; ++i)
    if (raw_full[i] != -1 && raw_full[i] != 0 && raw_full[i] != 100) return fail(HDSM_ERR_BAD_ARG, "a raw grid holds -1, 0 and 100 only");
  if (vox < 4 || vox >= ((size_t)1 << 30)) return fail(HDSM_ERR_BAD_ARG, "a raw world needs 4 .. 2^30 - 1 voxels");
  const int32_t zero[3] = {0, 0, 0};
  const size_t scr = hdsm_map_region_scratch_bytes(map_cfg, d->c.wdim, zero, d->c.wdim);  // the largest box; >= the full form's 2 vox
  if (scr == 0) return fail(HDSM_ERR_BAD_ARG, std::string("map configuration: ") + hdsm_map_last_error());
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  WorldEdits& w = d->edits;
  {  // out of the dswarm until the new grid is in it: an allocation or a copy that fails leaves no raw world resident
    DevBuf<int8_t> raw = std::move(w.d_raw);
    DevBuf<uint8_t> map_scr = std::move(w.d_map_scr);
    if (!raw) HIP_TRY(raw.alloc(vox));
    if (!map_scr) HIP_TRY(map_scr.alloc(scr));
    HIP_TRY(hipMemcpy(raw.get(), raw_full, vox, hipMemcpyHostToDevice));
    w.d_raw = std::move(raw), w.d_map_scr = std::move(map_scr);
  }
  // (the arguments were checked above: what can still fail is a launch, and then the device world is no longer the old one —
  // the cache is emptied on that way out too)
  const int rc = hdsm_map_preprocess_device(d->device, map_cfg, 1, d->c.wdim, w.d_raw.get(), d->d_world.get(), w.d_map_scr.get(), nullptr);
  if (rc == HDSM_OK) w.mcfg = *map_cfg;
  const int rc2 = invalidate(d, nullptr, nullptr, nullptr);
  if (rc) {
    w.d_raw.reset();  // (no raw world is resident: the raw update calls keep refusing)
    return fail(rc, std::string("hdsm_map_preprocess_device: ") + hdsm_map_last_error());
  }
  if (rc2) return rc2;
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

int hdsm_dswarm_update_world_raw_device(void* dswarm, const int8_t* d_raw_values, const int32_t lo[3], const int32_t bdim[3], void* hip_stream) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k < 0) return k;
  WorldEdits& w = d->edits;
  if (!w.d_raw) return fail(HDSM_ERR_BAD_ARG, "no raw world is resident (hdsm_dswarm_set_raw_world)");
  if (k == 0) return HDSM_OK;
  if (!d_raw_values) return fail(HDSM_ERR_BAD_ARG, "null values");
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int32_t wlo[3], wdim[3];
  if (int rc = hdsm_map_region_extent(&w.mcfg, d->c.wdim, lo, bdim, wlo, wdim, nullptr, nullptr)) return fail(rc, hdsm_map_last_error());
  if (int rc = put_box(d, d_raw_values, w.d_raw.get(), lo, bdim, st)) return rc;
  if (int rc = hdsm_map_preprocess_region_device(d->device, &w.mcfg, d->c.wdim, w.d_raw.get(), d->d_world.get(), lo, bdim, w.d_map_scr.get(), st))
    return fail(rc, std::string("hdsm_map_preprocess_region_device: ") + hdsm_map_last_error());
  if (int rc = invalidate(d, wlo, wdim, st)) return rc;
  ++w.updates, w.voxels += (long long)wdim[0] * wdim[1] * wdim[2];
  return HDSM_OK;
}

int hdsm_dswarm_update_world_raw(void* dswarm, const int8_t* raw_values, const int32_t lo[3], const int32_t bdim[3]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k < 0) return k;
  if (!d->edits.d_raw) return fail(HDSM_ERR_BAD_ARG, "no raw world is resident (hdsm_dswarm_set_raw_world)");
  if (k == 0) return HDSM_OK;
  if (!raw_values) return fail(HDSM_ERR_BAD_ARG, "null values");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = stage_box(d, raw_values, bdim)) return rc;
  if (int rc = hdsm_dswarm_update_world_raw_device(dswarm, d->edits.d_edit.get(), lo, bdim, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

int hdsm_dswarm_download_world(void* dswarm, int8_t* world) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !world) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return fail(HDSM_ERR_BAD_ARG, "the dswarm has no world");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(world, d->d_world.get(), (size_t)d->c.wdim[0] * d->c.wdim[1] * d->c.wdim[2], hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_world_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = static_cast<DSwarm*>(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->edits.updates, out[1] = d->edits.voxels, out[2] = 0, out[3] = d->edits.d_raw ? 1 : 0;
  if (!d->edits.d_dropped) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long n = 0;
  HIP_TRY(hipMemcpy(&n, d->edits.d_dropped.get(), sizeof n, hipMemcpyDeviceToHost));
  out[2] = (int64_t)n;
  return HDSM_OK;
}

}  // extern "C"
