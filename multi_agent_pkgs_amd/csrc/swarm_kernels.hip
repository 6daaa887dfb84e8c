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
//   k_command    (only with commands on, hdsm_dswarm_set_commands) the yaw step, the setpoints of the interval about to be flown and the
//                pose the round ends in (command_kernels.hip)                                    one lane per agent
//   k_vehicle    (only with a vehicle on, hdsm_dswarm_set_vehicle) every flown agent's quadrotor and controller fly those setpoints,
//                step_plan * n_sub sub-steps; state_curr, the track record and the pose take what it flew (vehicle_kernels.hip)
//                                                                                                one lane per flown agent
//   k_mission    (only with a mission on, hdsm_dswarm_set_mission) every flown agent's state judged against its waypoint: arrival, the
//                next goal and the due flag the next round's path step reads, stalls, the shard's tally (mission_kernels.hip)
//                                                                                                one lane per flown agent
//   exchange     ONE RCCL all-gather (hdsm_exchange_device), nothing on a single rank (k_commit publishes straight into the plans
//                buffer), or — the ranks of one process, hdsm_dswarm_round_ranks — ONE k_gather_local per rank (exchange_kernels.hip)
// The per-agent functions are the SAME source as the host mirror (swarm_core.h), which is how the two loops are compared in
// tests/test_gpu_configs.py. AC = multi_agent_planner/src/agent_class.cpp of the reference.
// This file is the round and nothing else: its kernels, its phases, hdsm_dswarm_create / _destroy / _round / _round_ranks and the phase
// timing. What runs BETWEEN rounds lives in dswarm_world.hip, dswarm_audit.hip, dswarm_flight.cpp and dswarm_models.cpp (dswarm.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "command_device.h"
#include "dswarm.h"
#include "hdsm_internal.h"
#include "link_core.h"
#include "mission_device.h"
#include "path_core.h"
#include "script_device.h"
#include "track_device.h"
#include "vehicle_device.h"

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

using namespace hdsm_dswarm;

namespace {
thread_local std::string g_err;
}
int hdsm_dswarm::fail(int code, const std::string& m) {
  g_err = m;
  return code;
}

// every event a timed round records (hdsm_dswarm_set_phase_timing; _set_audit and _set_history when the timing is already on)
int hdsm_dswarm::timing_events(DSwarm* d) {
  for (hdsm_mem::DevEvent& e : d->ev) HIP_TRY(e.create());
  HIP_TRY(d->path.timed.create());
  HIP_TRY(d->audit.timed.create());
  return HDSM_OK;
}

namespace {

// scratch of one agent's voxel decompositions, in LDS (dynamic shared memory of k_corridor): the workspace, the overlay bits and
// the 2-bit cache of the world under the overlay. The decomposition is one lane's chain of small dependent accesses — in global
// memory every one of them was a round trip (33 ms per round for 256 agents in the pillar forest).
constexpr size_t SLAB = hdsm_cd::WAVE_LDS_MAX;  // (the launch asks for what its n_it needs: wave_lds_bytes)
// k_corridor also has static __shared__ state (the walk's rows and flags, < 4 KB); together they must stay inside the 64 KB a
// kernel may use without hipFuncAttributeMaxDynamicSharedMemorySize — a growth of Work / the overlay fails HERE, not at launch
static_assert(SLAB + 4096 <= 64 * 1024, "k_corridor: dynamic + static LDS exceed the default 64 KB limit");

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
__device__ __forceinline__ void path_agent(const Cfg& c, int k, AgentS* agents, const double* goals, unsigned long long* cnt, hdsm_path::PathLds& lds,
                                           int tid) {
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
__global__ __launch_bounds__(hdsm_path::THREADS) void k_path(Cfg c, const int32_t* idx, AgentS* agents, const double* goals,
                                                              unsigned long long* cnt) {
  __shared__ hdsm_path::PathLds lds;
  path_agent(c, idx != nullptr ? idx[blockIdx.x] : (int)blockIdx.x, agents, goals, cnt, lds, (int)threadIdx.x);
}
// k_path sized on the device (only while a mission is on, hdsm_dswarm_set_mission): launched over the flown agents; the workgroup of an
// agent whose due flag (k_mission) is not set returns at once, before it touches LDS — unless `all`, a round of the path period. The
// flag is cleared when the agent is planned (behind the barrier every thread passes after reading it). planned (or NULL in an `all`
// round, which the host counts): [0] the agents these launches planned, [1] the number `seq` (> 0) of the last launch that planned
// somebody, [2] how many launches did — the first workgroup of a launch to plan finds another number in [1] and counts the launch.
__device__ __forceinline__ void count_planned(unsigned long long* planned, unsigned long long seq) {
  if (planned == nullptr) return;
  atomicAdd(&planned[0], 1ull);
  if (atomicExch(&planned[1], seq) != seq) atomicAdd(&planned[2], 1ull);
}
__global__ __launch_bounds__(hdsm_path::THREADS) void k_due_path(Cfg c, int all, uint8_t* flag, AgentS* agents, const double* goals,
                                                                  unsigned long long* cnt, unsigned long long* planned, unsigned long long seq) {
  __shared__ hdsm_path::PathLds lds;
  const int k = (int)blockIdx.x;
  if (!all && flag[k] == 0) return;
  path_agent(c, k, agents, goals, cnt, lds, (int)threadIdx.x);
  if (threadIdx.x == 0) {
    flag[k] = 0;
    count_planned(planned, seq);
  }
}

// k_path in clearance mode (path_core.h, 6a-7': the distance-map planner and ShortenDMPPath after the descent); rn, rows: the tunnel's
// mask (hdsm_path::DmpMask). The same bookkeeping as k_path.
__device__ __forceinline__ void dmp_agent(const Cfg& c, int k, AgentS* agents, const double* goals, unsigned long long* cnt, int rn,
                                          const uint32_t* rows, hdsm_path::DmpLds& lds, int tid) {
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
__global__ __launch_bounds__(hdsm_path::THREADS) void k_dmp(Cfg c, const int32_t* idx, AgentS* agents, const double* goals,
                                                             unsigned long long* cnt, int rn, const uint32_t* rows) {
  __shared__ hdsm_path::DmpLds lds;
  dmp_agent(c, idx != nullptr ? idx[blockIdx.x] : (int)blockIdx.x, agents, goals, cnt, rn, rows, lds, (int)threadIdx.x);
}
// k_dmp sized on the device: as k_due_path
__global__ __launch_bounds__(hdsm_path::THREADS) void k_due_dmp(Cfg c, int all, uint8_t* flag, AgentS* agents, const double* goals,
                                                                 unsigned long long* cnt, unsigned long long* planned, unsigned long long seq, int rn,
                                                                 const uint32_t* rows) {
  __shared__ hdsm_path::DmpLds lds;
  const int k = (int)blockIdx.x;
  if (!all && flag[k] == 0) return;
  dmp_agent(c, k, agents, goals, cnt, rn, rows, lds, (int)threadIdx.x);
  if (threadIdx.x == 0) {
    flag[k] = 0;
    count_planned(planned, seq);
  }
}

// One link round (link_core.h, deliver_slot): a wavefront per slot of the plans buffer, four per workgroup. No LDS, no atomics: a
// slot is touched by its own wavefront alone.
__global__ __launch_bounds__(256) void k_deliver(hdsm_link::Round a) {
  const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (k >= a.G) return;
  hdsm_link::deliver_slot(a, k, (int)threadIdx.x & 63, 64);
}

// every buffer a round of n_local agents in a world of hworld's size needs, zero-filled
hipError_t alloc_round_buffers(DSwarm* d, const int8_t* hworld) {
  const Cfg& c = d->c;
  const size_t n = (size_t)d->n_local, L = (size_t)d->per, G = (size_t)d->slots(), N = (size_t)c.N, P = (size_t)c.P, RS = (size_t)c.RS,
               REC = (size_t)d->rec();
  hdsm_mem::FirstError ok;
  ok(d->d_agents.alloc_zeroed(n));
  if (hworld) {
    ok(d->d_world.alloc_zeroed(d->voxels()));
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
  p.timed.valid = false;
  if (Mission& ms = d.mission; ms.on) {
    // a mission is on: who is due is on the device (k_mission's flags). ONE launch over the flown agents; a workgroup that is not
    // flagged returns at once. No host round trip decides this.
    if (const int n_fly = d.n_fly(); n_fly > 0) {
      if (d.phase_timing) HIP_TRY(p.timed.record_start(st));
      // hdsm_dswarm_path_stats keeps counting the launches that planned somebody: an `all` round here, a device-sized one on the device
      unsigned long long* const planned = all ? nullptr : ms.d_planned.get();
      const unsigned long long seq = (unsigned long long)ms.path_launches + 1ull;
      if (p.dmp)
        hipLaunchKernelGGL(k_due_dmp, dim3((unsigned)n_fly), dim3(hdsm_path::THREADS), 0, st, d.c, all ? 1 : 0, ms.d_flag.get(), d.d_agents.get(),
                           p.d_goals.get(), p.d_cnt.get(), planned, seq, p.dmp_rn, p.d_dmp_rows.get());
      else
        hipLaunchKernelGGL(k_due_path, dim3((unsigned)n_fly), dim3(hdsm_path::THREADS), 0, st, d.c, all ? 1 : 0, ms.d_flag.get(), d.d_agents.get(),
                           p.d_goals.get(), p.d_cnt.get(), planned, seq);
      HIP_TRY(hipGetLastError());
      if (d.phase_timing) HIP_TRY(p.timed.record_stop(st));
      if (all) ++p.launches;
      else ++ms.path_launches;
    }
    ++p.round;
    return HDSM_OK;
  }
  int n_plan = all ? d.n_fly() : p.n_due;
  if (!all && d.script.n > 0) {  // (the list of the due agents ascends: the flown ones come first)
    n_plan = 0;
    for (int k = 0; k < d.n_fly(); ++k) n_plan += p.due[(size_t)k] != 0;
  }
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
  const int n = d.n_fly(), G = d.slots();
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
                     d.d_ctrl.get(), d.d_used.get(), d.d_status.get(), d.publish_to(direct), d.d_fails.get(),
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
    HIP_TRY(hdsm_script::launch(hdsm_script::Round{s.n, s.n_knots, d.c.N, d.c.step_plan, s.predict, s.round, d.prm.dt, s.d_knots.get(),
                                                   d.publish_to(direct) + (size_t)n_fly * d.rec(),
                                                   direct ? d.d_has.get() + n_fly : nullptr, d.d_status.get() + n_fly, d.d_agents.get() + n_fly},
                                st));
    ++s.round, ++s.launches;
  }
  if (Commands& m = d.cmd; m.on && d.n_local > 0) {  // what the vehicles are told (inside phase [5]). ONE launch behind the commit: state_curr
    // of before it still stands in the solver's x_0 input, this round's reference in the reference buffer
    hdsm_cmd::Launch a{};
    a.n = d.n_local, a.n_fly = n_fly, a.N = d.c.N, a.step_plan = d.c.step_plan, a.yaw_idx = m.yaw_idx, a.dt = d.prm.dt, a.k_p_yaw = m.k_p_yaw;
    a.agents = d.d_agents.get(), a.status = d.d_status.get(), a.before = d.d_state.get(), a.ref_full = d.d_ref_full.get();
    a.yaw = m.d_yaw.get(), a.setpoint = m.d_setpoint.get(), a.pose = m.d_pose.get(), a.cnt = m.d_cnt.get();
    HIP_TRY(hdsm_cmd::launch(a, st));
    ++m.launches;
  }
  if (Vehicle& v = d.veh; v.on) {  // the flown agents' vehicles fly the setpoints just written (inside phase [5]); state_curr takes what they flew
    if (n_fly > 0) {
      hdsm_veh::Launch a{};
      a.n = n_fly, a.step_plan = d.c.step_plan, a.q = v.q, a.dt = d.prm.dt, a.m = v.m;
      a.agents = d.d_agents.get(), a.records = d.track.d_rec.get(), a.setpoint = d.cmd.d_setpoint.get(), a.vstate = v.d_state.get();
      a.pose = d.cmd.d_pose.get(), a.cnt = v.d_cnt.get();
      HIP_TRY(hdsm_veh::launch(a, st));
      ++v.launches;
    }
    ++v.q;
  }
  if (Mission& ms = d.mission; ms.on) {  // what the flown agents flew is judged against their waypoints (the last launch of phase [5]): an
    // arrival writes the next goal into the path step's goal buffer and flags the agent for the next round's path step
    if (n_fly > 0) {
      HIP_TRY(hdsm_mission_rule::launch(hdsm_mission_rule::Launch{n_fly, 0, ms.q, ms.m, d.d_agents.get(), nullptr, ms.d_wps.get(), ms.d_count.get(),
                                                                  ms.d_rec.get(), d.path.d_goals.get(), ms.d_flag.get(), ms.d_tally.get()},
                                        st));
      ++ms.launches;
    }
    ++ms.q;
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
  return hdsm_link::Round{d.slots(), d.n_rob, d.c.N, d.c.step_plan, l.n_rounds, l.D, l.time_aware, l.round, l.d_fate.get(), d.d_plans.get(),
                          l.d_ring.get(), l.d_seen.get(), l.d_seen_has.get(), l.d_seen_round.get(), l.d_shift.get(), l.d_cnt.get()};
}
int deliver(DSwarm& d, hipStream_t st) {
  Links& l = d.links;
  const int G = d.slots();
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

// Where a round of the device-resident loop goes, measured with HIP events on the round's own stream: the records sit between the
// launches of hdsm_dswarm_round — [0] k_corridor, [1] k_vel_cap, [2] hdsm_reference_device (pack + reference), [3] k_keep_free,
// [4] hdsm_replan_device (pre-pass, solver kernels, merge), [5] k_commit, [6] the exchange. hdsm_dswarm_last_phase_ms synchronises
// with the last timed round and returns the seven durations in milliseconds (a phase the round did not launch: ~0).
int hdsm_dswarm_set_phase_timing(void* dswarm, int32_t on) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  HIP_TRY(hipSetDevice(d->device));
  if (on)
    if (int rc = timing_events(d)) return rc;
  d->phase_timing = on != 0, d->phase_valid = false, d->path.timed.valid = false, d->audit.timed.valid = false;
  return HDSM_OK;
}

int hdsm_dswarm_last_phase_ms(void* dswarm, float ms[7]) {
  DSwarm* d = as_dswarm(dswarm);
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
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !ms) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->phase_valid) return fail(HDSM_ERR_BAD_ARG, "no round has run with hdsm_dswarm_set_phase_timing on");
  *ms = 0.0f;
  if (!d->path.timed.valid) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(d->path.timed.ms(ms));
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
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return;
  (void)device_idle(d);
  delete d;
}

int hdsm_dswarm_round(void* dswarm, void* comm, void* hip_stream) {
  DSwarm* d = as_dswarm(dswarm);
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
  const DSwarm* d0 = as_dswarm(dswarms[0]);
  if (int rc = hdsm_internal_local_check(world, comms, d0->rec())) return fail(rc, std::string("hdsm_dswarm_round_ranks: ") + hdsm_last_error());
  std::vector<const double*> send((size_t)world);
  for (int r = 0; r < world; ++r) {
    const DSwarm* d = as_dswarm(dswarms[r]);
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
    DSwarm* d = as_dswarm(dswarms[r]);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = static_cast<hipStream_t>(hip_streams ? hip_streams[r] : nullptr);
    DoneOnce done_once(d->solver, st);
    if (int rc = round_front(*d, comms[r], st)) return rc;
  }
  for (int r = 0; r < world; ++r) {
    DSwarm* d = as_dswarm(dswarms[r]);
    HIP_TRY(hipSetDevice(d->device));
    if (int rc = round_back(*d, comms[r], comms[r], static_cast<hipStream_t>(hip_streams ? hip_streams[r] : nullptr))) return rc;
  }
  return HDSM_OK;
}

}  // extern "C"
