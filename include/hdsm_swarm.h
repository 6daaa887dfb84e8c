/*
 * hdsm_swarm.h — host-side planner state of a shard of agents, driving hdsm_replan() in closed loop.
 *
 * This is the part of multi_agent_planner::Agent that sits directly around the solve in
 * Agent::TrajPlanningIteration (AC:157-258), restated for a BATCH of agents and for the obstacle-free
 * environments of BASELINE configs 1, 2 and 4 (circle exchange, empty world):
 *
 *   hdsm_swarm_prepare()  = GenerateSafeCorridor (AC:1236-1447, with the free-space polyhedron of
 *                           convex_decomp.cpp:54-373 in closed form: SURVEY.md App. D.2)
 *                         + GenerateReferenceTrajectory (AC:1449-1553; SamplePath AC:1591-1663,
 *                           ComputePathVelocity's neighbour term AC:1769-1801, GetVelocityLimit AC:1805-1817)
 *                         -> the input arrays of hdsm_replan / hdsm_replan_device
 *   hdsm_swarm_commit()   = read-back bookkeeping (poly_used_idx_), the shift-by-one fallback on failure
 *                           (AC:1000-1019), CheckReferenceTrajIncrement (AC:569-585, GetPathProgress
 *                           path_tools.cpp:419-479), state advance (AC:233-238), and the record this shard
 *                           publishes (PublishTrajectoryFull AC:645-677) for the next all-gather.
 *
 * Simplifications, stated: the global path is the straight segment start->goal (what JPS+DMP returns in
 * an empty world up to voxel snapping); the voxel grid is all-free, so the potential
 * field term of ComputePathVelocity is inactive and KeepOnlyFreeReference is the identity.
 * Pure host code; arrays use the layouts of hdsm.h.
 */
#ifndef HDSM_SWARM_H
#define HDSM_SWARM_H

#include <stddef.h>

#include "hdsm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdsm_swarm_config {
  double path_vel_min, path_vel_max; /* agent_agile_config.yaml: 4.5 / 9.0                                */
  double sens_dist, sens_pot;        /* 0.05 / 0.18                                                       */
  double sens_other_agents;          /* default 1.0 (AC:2213)                                             */
  double path_vel_dec;               /* 0.0                                                               */
  double thresh_dist;                /* 1.0                                                               */
  double voxel_size;                 /* 0.3                                                               */
  double grid_range[3];              /* local grid extent, 20 x 20 x 6 m                                  */
  double grid_z_min;                 /* z of the local grid origin (ground), 0.0                          */
  int32_t n_it_decomp;               /* 42 -> 7 voxel layers per face                                     */
  int32_t step_plan;                 /* 1                                                                 */
  int32_t use_cvx_new;               /* use_cvx_new_ (AC:2222, shipped: false): always use the shape-aware decomposition;
                                        0 = only where the seed is pinched between occupied voxels (AC:1385-1395)      */
  int32_t reserved0;
} hdsm_swarm_config;

void hdsm_swarm_default_config(hdsm_swarm_config* cfg);

/* Agents [first_id, first_id + n_local) of a swarm of n_rob. starts/goals: [n_local][3] (state_ini, goal). */
int hdsm_swarm_create(const hdsm_params* prm, const hdsm_swarm_config* cfg, int32_t n_rob, int32_t first_id,
                      int32_t n_local, const double* starts, const double* goals, void** swarm);
void hdsm_swarm_destroy(void* swarm);

/* Fills the solver inputs of this round for the n_local agents from the all-gathered plans of last round. */
int hdsm_swarm_prepare(void* swarm, const double* plans_all, const uint8_t* has_plan, int32_t* agent_id,
                       double* state_curr, double* traj_ref, int32_t* n_poly, int32_t* n_rows_static,
                       double* A_static, double* b_static);

/* Consumes the solver outputs; writes the shard's published plans [n_local][N+1][9] and has_plan flags. */
int hdsm_swarm_commit(void* swarm, const double* traj_out, const double* ctrl_out, const uint8_t* poly_used,
                      const int32_t* status, double* plans_local, uint8_t* has_plan_local);

/* f1 on the device: (1) hdsm_swarm_reference_inputs() exports, for every local agent, the polyline
 * GenerateReferenceTrajectory would sample this round (AC:1459-1496: the starting point taken from the previous
 * reference, then the rest of the global path): path[n_local][3][3], n_path[n_local]; (2) the caller runs
 * hdsm_reference / hdsm_reference_device; (3) hdsm_swarm_set_reference() hands the result back — the next
 * hdsm_swarm_prepare() then uses it instead of generating the reference on the host.                        */
int hdsm_swarm_reference_inputs(void* swarm, double* path, int32_t* n_path);
/* vel_cap[n_local] for hdsm_reference*: the voxel / potential-field term of ComputePathVelocity (AC:1709-1766: raycast of the
 * polyline through the agent's local grid, GetVelocityLimit of every voxel crossed) on the world of hdsm_swarm_set_world;
 * path_vel_max in free space. hdsm_swarm_set_reference then applies KeepOnlyFreeReference (AC:1665-1693) to what comes back.
 * (The device-resident loop does both on the device: k_vel_cap, k_keep_free.) */
int hdsm_swarm_vel_cap(void* swarm, double* vel_cap);
int hdsm_swarm_set_reference(void* swarm, const double* ref_full, const double* path_vel);

/* Next row f2: an occupied world. occupancy [dim[2]][dim[1]][dim[0]] int8 (x fastest), voxels of cfg.voxel_size,
 * >= 100 occupied (already inflated by the drone radius — the map builder's job, f4); origin = world position of
 * voxel (0,0,0), a multiple of the voxel size so that the agents' local grids register with it. From then on
 * hdsm_swarm_prepare() cuts each agent's local grid (20 x 20 x 6 m around it) out of this world and builds the
 * corridor polyhedra with hdsm_poly_octa3d instead of the free-space closed form; with an empty world both give
 * the same polyhedra. NULL occupancy = back to free space. The global path stays the straight segment
 * start -> goal (f3, JPS + DMP, is not built): the caller is responsible for worlds in which that is collision-free. */
int hdsm_swarm_set_world(void* swarm, const int8_t* occupancy, const int32_t dim[3], const double origin[3]);
/* A map update (ABI 1.7; VoxelGridResponseCallback / MappingUtilVoxelGridCallback, AC:2310-2378, for the shared world): the box
 * lo[3] .. lo + bdim[3] (world voxels, x y z) of the PROCESSED world given to hdsm_swarm_set_world takes values
 * [bdim[2]][bdim[1]][bdim[0]] as they are. From the next hdsm_swarm_prepare / _prepare_corridor / path step on everything reads the new
 * voxels, exactly as after hdsm_swarm_set_world of the edited grid. Polyhedra an agent keeps (AC:1253-1282) are not checked against
 * the new voxels — the reference keeps them too — and global paths adapt only through the path step (its period, a goal change,
 * hdsm_swarm_replan_paths): an edit plans nothing by itself. HDSM_ERR_BAD_ARG without a world or for a box not inside it; an empty
 * box is a no-op. */
int hdsm_swarm_update_world(void* swarm, const int8_t* values, const int32_t lo[3], const int32_t bdim[3]);

/* Next row f2, first piece — the convex voxel decomposition GenerateSafeCorridor calls for every seed
 * (convex_decomp_lib::GetPolyOcta3D, convex_decomp_util/src/convex_decomp.cpp:5-376): a cuboid of free voxels grown
 * from `seed` face by face (n_it face turns, order -y +x +y -x +z -z), chamfered with integer slopes where obstacles
 * cut an edge.
 *   grid  [dim[2]][dim[1]][dim[0]] int8, x fastest: < 100 free, >= 100 occupied (CVX_DCMP_OCC); voxels taken by the
 *         polyhedron are overwritten with `mark` (the reference's CONV: a negative value, one per polyhedron)
 *   rows  [max_rows][4] = (n, n . p): n . x <= n . p; chamfers first, then the six faces; at most 18 rows
 * Returns HDSM_ERR_CAPACITY (and the needed count in n_rows) if max_rows is too small.                        */
int hdsm_poly_octa3d(const int32_t seed[3], int8_t* grid, const int32_t dim[3], int32_t n_it, double res,
                     int32_t mark, const double origin[3], double* rows, int32_t max_rows, int32_t* n_rows);
/* The shape-aware variant, convex_decomp_lib::GetPolyOcta3DNew (convex_decomp.cpp:590-1160, helpers FindCorners :378-564 and
 * SideIsEmpty :577-588): same growth, but a chamfer only starts where an obstacle really lies behind it, a layer that
 * covers less than half of its allowance is skipped, and layers may reach the last voxel of the grid. GenerateSafeCorridor
 * switches to it when the seed is pinched between two occupied voxels along an axis (AC:1385-1395). Same arguments; voxels
 * with a positive value below 100 (potential field) are free for the growth but count as "not empty" for the chamfer test. */
int hdsm_poly_octa3d_new(const int32_t seed[3], int8_t* grid, const int32_t dim[3], int32_t n_it, double res,
                         int32_t mark, const double origin[3], double* rows, int32_t max_rows, int32_t* n_rows);

/* Row f2 on the device: a BATCH of decompositions on local grids that are windows into one world grid (csrc/corridor_kernels.hip;
 * one thread per seed, the same source as the two host functions above, rows bit-identical to theirs). For seed t:
 *   off[t][3]      local voxel (0,0,0) in world voxels; ldim = dimensions of every local grid
 *   ground_k[t]    local voxels with k < ground_k are unknown -> occupied (AC:1302, 1307); unknown (negative) world voxels are
 *                  occupied, voxels outside the world are free (what hdsm_swarm_set_world's host path does)
 *   seed[t][3]     local voxel; variant[t] 0 = GetPolyOcta3D, 1 = GetPolyOcta3DNew, -1 = decide like AC:1385-1395
 *   origin[t][3]   world position of local voxel (0,0,0)
 *   rows[t][max_rows][4], n_rows[t], rc[t] (hdsm_error per seed), cells[t] (voxels of the polyhedron; may be NULL)
 * hdsm_poly_octa3d_batch: host pointers (copies the world in, PCIe-inclusive). hdsm_poly_octa3d_device: device pointers,
 * asynchronous on hip_stream, `scratch` = hdsm_poly_octa3d_scratch_bytes(n) bytes of device memory. */
int hdsm_poly_octa3d_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                           const int32_t* off, const int32_t* ground_k, const int32_t* seed, const int32_t* variant,
                           const double* origin, int32_t n_it, double res, double* rows, int32_t max_rows, int32_t* n_rows,
                           int32_t* rc, int32_t* cells);
int hdsm_poly_octa3d_device(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                            const int32_t* off, const int32_t* ground_k, const int32_t* seed, const int32_t* variant,
                            const double* origin, int32_t n_it, double res, double* rows, int32_t max_rows, int32_t* n_rows,
                            int32_t* rc, int32_t* cells, void* scratch, void* hip_stream);
size_t hdsm_poly_octa3d_scratch_bytes(int32_t n);
/* The same batch with ONE WAVEFRONT per seed (workspace in LDS, the 64 lanes run the decomposition cooperatively — the form the
 * device-resident loop uses for one agent's seeds): lower latency per seed, fewer seeds in flight, no scratch; same results. */
int hdsm_poly_octa3d_batch_wave(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                                const int32_t* off, const int32_t* ground_k, const int32_t* seed, const int32_t* variant,
                                const double* origin, int32_t n_it, double res, double* rows, int32_t max_rows, int32_t* n_rows,
                                int32_t* rc, int32_t* cells);
int hdsm_poly_octa3d_device_wave(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                                 const int32_t* off, const int32_t* ground_k, const int32_t* seed, const int32_t* variant,
                                 const double* origin, int32_t n_it, double res, double* rows, int32_t max_rows, int32_t* n_rows,
                                 int32_t* rc, int32_t* cells, void* hip_stream);
const char* hdsm_corridor_last_error(void);

/* Global paths (path_curr_ of the reference, produced there by the path thread: JPS + DMP + shortening, AC:261-567 — out of
 * scope as such). Default: the straight segment start -> goal. hdsm_swarm_set_paths installs caller-supplied polylines
 * [n_local][pmax][3] with n_path[k] >= 2 points each (first = start, last = goal). hdsm_swarm_route computes them on the
 * world given to hdsm_swarm_set_world: a minimal collision-free router (3-D A* over free voxels, 26-connected, extra cost next
 * to obstacles, then greedy line-of-sight shortening) — NOT the reference's JPS3D / distance-map planner, only something
 * that lets BASELINE's forest configurations fly. hdsm_swarm_get_paths reads the current paths back (n_path > pmax -> CAPACITY).
 * Both corridor generation (AC:1286-1290) and reference sampling (AC:1459-1496) then walk these polylines. */
int hdsm_swarm_set_paths(void* swarm, const double* paths, const int32_t* n_path, int32_t pmax);
int hdsm_swarm_route(void* swarm, int32_t* n_failed);
int hdsm_swarm_get_paths(void* swarm, int32_t pmax, double* paths, int32_t* n_path);
/* hdsm_swarm_reference_inputs for paths with more than two points: path[n_local][pmax][3]; a polyline longer than pmax is
 * cut after pmax points, which changes nothing as long as the kept part is longer than n_hor * path_vel_max * dt (checked:
 * otherwise HDSM_ERR_CAPACITY). */
int hdsm_swarm_reference_inputs_n(void* swarm, int32_t pmax, double* path, int32_t* n_path);
/* ---- the path step (ABI 1.4): Agent::UpdatePath (AC:261-454) and GoalCallback (AC:2380-2388) ----------------------------------
 * A stated stand-in for the reference's JPS3D + DMP + ShortenDMPPath (csrc/path_core.h; not its output): on the agent's local grid
 * (the corridor's window of the world, ClearBoundary AC:1819-1854 applied), from S = the point the reference polyline starts from this
 * round towards GetIntermediateGoal(goal) (AC:1891-1941): a 6-connected BFS from the goal voxel, a descent from the start voxel, a
 * greedy line-of-sight shortening with the reference's Raycast. With no world the path is [S, goal]. Status per agent: 0 a new path
 * (replaces path_curr_), 1 no free voxel within 6 of the start or goal voxel, 2 goal unreachable in the local grid, 3 more than 48
 * points, 4 local grid or descent beyond the device workspace. On a non-zero status the agent keeps its path.
 *   hdsm_swarm_set_goals        goals [n_local][3]; the agents whose goal changed plan a new path at the start of the next round
 *   hdsm_swarm_set_path_period  0 (default) never; k: every agent plans a new path every k-th round, the first at the next round.
 *                               The step runs at the start of a round, before the corridor, in whichever of
 *                               hdsm_swarm_prepare_corridor / hdsm_swarm_prepare builds the corridor. The period and the round phase
 *                               go into hdsm_dswarm_create and come back with hdsm_dswarm_download(swarm).
 *   hdsm_swarm_replan_paths     every local agent now; n_failed (may be NULL) = agents with a non-zero status
 *   hdsm_swarm_path_errors      agents whose last path step failed; codes[n_local] (may be NULL) the status per agent
 * The stand-alone batch (hdsm_poly_octa3d_batch's pattern): for case t the local grid ldim at off[t] in the world (wdim, NULL = free
 * space), ground_k[t], origin[t][3], start[t][3], goal[t][3], voxel size res -> paths[t][pmax][3] (rows beyond n_path[t] repeat the
 * last point; zeros on failure), n_path[t], status[t]. hdsm_local_path_batch plans on `device` (one workgroup per case, host pointers
 * in and out), hdsm_local_path_host on the CPU; the two agree bit for bit. HDSM_ERR_CAPACITY if some n_path > pmax.          */
int hdsm_swarm_set_goals(void* swarm, const double* goals);
int hdsm_swarm_set_path_period(void* swarm, int32_t period);
int hdsm_swarm_replan_paths(void* swarm, int32_t* n_failed);
int hdsm_swarm_path_errors(void* swarm, int32_t* codes);
int hdsm_local_path_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                          const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res, int32_t pmax,
                          double* paths, int32_t* n_path, int32_t* status);
int hdsm_local_path_host(int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                         const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res, int32_t pmax,
                         double* paths, int32_t* n_path, int32_t* status);
/* ---- the path step's clearance mode (ABI 1.5): the reference's distance-map planner and ShortenDMPPath ---------------------------
 * Opt-in. The BFS descent above stays as the stand-in for the JPS raw path; what follows it is the reference's (csrc/path_core.h,
 * 6a-7'): the distance-map planner (a shortest path in a tunnel of radius search_rad round the descent, a step into voxel v costs
 * 1 + v's potential 1..99, 6-connected, one iteration) and ShortenDMPPath (corners are cut only between points in potential-free
 * voxels along rays that visit potential-free voxels alone). Status 4 also when the tunnel is wider than 15 voxels or holds more
 * than 87168 voxels.
 *   hdsm_swarm_set_path_clearance  search_rad 0 (default): off, the plain step. Non-zero: hdsm_swarm_replan_paths, the path period
 *                                  and goal changes plan in clearance mode; < 0: no tunnel (every free voxel of the local grid). The
 *                                  reference ships 1.8 (dmp_search_rad). HDSM_ERR_BAD_ARG for a radius over 15 voxels. The setting
 *                                  goes into hdsm_dswarm_create like the path period.
 *   hdsm_local_path_dmp_batch / _host  hdsm_local_path_batch / _host in clearance mode: the same arguments plus search_rad, and
 *                                  cost[t] (the path's cost: the sum of 1 + potential over its steps plus the start voxel's
 *                                  potential; -1 on failure) and n_raw[t] (voxels of the planner's chain, 0 on failure). The two
 *                                  agree bit for bit.                                                                        */
int hdsm_swarm_set_path_clearance(void* swarm, double search_rad);
int hdsm_local_path_dmp_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                              const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res,
                              double search_rad, int32_t pmax, double* paths, int32_t* n_path, int32_t* status, int32_t* cost, int32_t* n_raw);
int hdsm_local_path_dmp_host(int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                             const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res,
                             double search_rad, int32_t pmax, double* paths, int32_t* n_path, int32_t* status, int32_t* cost, int32_t* n_raw);

/* Number of local agents whose corridor generation failed in the last hdsm_swarm_prepare (seed outside the local grid, or a
 * polyhedron with more rows than max_rows_static); codes[n_local] (may be NULL) receives the hdsm_error per agent. Those
 * agents kept the polyhedra they had. */
int hdsm_swarm_corridor_errors(void* swarm, int32_t* codes);

/* GenerateSafeCorridor alone (AC:165). With the reference generated elsewhere (hdsm_reference*, row f1) the reference's own order
 * is: corridor from the PREVIOUS reference, then the new reference, then the solve — call this first, then
 * hdsm_swarm_reference_inputs* / hdsm_reference* / hdsm_swarm_set_reference, then hdsm_swarm_prepare (which then skips the corridor). */
int hdsm_swarm_prepare_corridor(void* swarm);

/* ---- the device-resident closed loop ------------------------------------------------------------------------------------------
 * The planner state of the shard moves into HBM (hdsm_dswarm_create copies it out of a host mirror that has been set up —
 * starts, goals, world, paths — and possibly flown for some rounds) and one replan round becomes a chain of launches on one
 * stream with no host round trip (csrc/swarm_kernels.hip; the calls between rounds: csrc/dswarm_*):
 *   corridor (AC:1236-1447, row f2 on the device) -> reference (row f1) -> solver inputs -> hdsm_replan_device -> commit
 *   (AC:960-1019, 569-585, 233-238) -> published records -> ONE RCCL all-gather (hdsm_exchange_device; a copy on a single rank).
 * `solver` is an hdsm handle with max_instances >= the shard and n_rob_max >= world_size * ceil(n_rob / world_size); `comm` an
 * hdsm_comm (NULL when world_size == 1). hdsm_dswarm_round is asynchronous on hip_stream. hdsm_dswarm_download synchronises
 * and copies out what the caller asks for (any pointer may be NULL): the agent states back into the host mirror `swarm`
 * (so that every hdsm_swarm_* diagnostic works on them), the all-gathered plans [world_size * per][N+1][9] and flags, the
 * statuses of the last round, the number of instances without solution so far.
 * The world and the configuration are those of the host mirror at hdsm_dswarm_create; the configuration stays fixed for the dswarm's
 * life, the world changes only through hdsm_dswarm_update_world* / _set_raw_world (ABI 1.7, below); the
 * global paths are fixed too, unless the path step is on (hdsm_swarm_set_path_period, hdsm_dswarm_set_goals: see below) (the
 * device corridor keeps each agent's last polyhedra and forms the rows of one that is asked for again from them instead of
 * growing it again — same rows, bit for bit; environment HDSM_POLY_CACHE=0 switches that off, for A/B runs). */
int hdsm_dswarm_create(void* swarm, void* solver, int32_t device, int32_t world_size, void** dswarm);
/* the all-gathered plans [n_rob][N+1][9] and flags [n_rob] the next round starts from (a swarm taken over in mid-flight) */
int hdsm_dswarm_upload_plans(void* dswarm, const double* plans_all, const uint8_t* has_plan);
int hdsm_dswarm_round(void* dswarm, void* comm, void* hip_stream);
int hdsm_dswarm_download(void* dswarm, void* swarm, double* plans_all, uint8_t* has_plan, int32_t* status, int32_t* failed_total);
void hdsm_dswarm_destroy(void* dswarm);
const char* hdsm_dswarm_last_error(void);
/* Where a round goes (a measurement aid; the reference books the same intervals per agent, AC:165-227 comp_time_sc_ / _tasc_ / _opt_):
 * with timing on, hdsm_dswarm_round records HIP events on its stream between its launches; hdsm_dswarm_last_phase_ms waits for the
 * last timed round and returns milliseconds of [0] k_corridor (GenerateSafeCorridor, AC:1236-1447), [1] k_vel_cap (ComputePathVelocity's
 * voxel term, AC:1709-1766), [2] hdsm_reference_device (AC:1449-1553), [3] k_keep_free (AC:1665-1693), [4] hdsm_replan_device
 * (AC:1086-1215 + 858-1023), [5] k_commit (AC:955-1019, 569-585, 233-238; with a tracking model k_track, with scripted agents k_script, with commands k_command behind it, all below), [6] the exchange
 * (AC:610-677; one rank: nothing).
 * Every record is a barrier packet in front of the next launch: a timed round is a few microseconds longer than a plain one. */
int hdsm_dswarm_set_phase_timing(void* dswarm, int32_t on);
int hdsm_dswarm_last_phase_ms(void* dswarm, float ms[7]);
/* The device corridor's polyhedron cache since hdsm_dswarm_create, summed over the shard: out[0] polyhedra asked for, out[1] formed
 * from a structure recorded in the same local grid, out[2] from one recorded in another grid at the same height (the interior
 * rule), out[3] 1 if the cache is on (a world is set and HDSM_POLY_CACHE is not 0). Synchronises the device. */
int hdsm_dswarm_cache_stats(void* dswarm, int64_t out[4]);

/* The path step on the device (k_path: one workgroup per due agent, the BFS as bit planes in LDS; launched before k_corridor only
 * in rounds where some agent is due). hdsm_dswarm_set_goals: goals [n_local][3], the changed agents plan at the next round
 * (synchronises the device). hdsm_dswarm_path_stats: out[0] agents planned, out[1] of them failed, out[2] launches of k_path since
 * hdsm_dswarm_create (synchronises). hdsm_dswarm_last_path_ms: with phase timing on, the duration of the last timed round's k_path
 * (0 if that round planned nothing); hdsm_dswarm_last_phase_ms's [0] k_corridor starts after it. */
int hdsm_dswarm_set_goals(void* dswarm, const double* goals);
int hdsm_dswarm_path_stats(void* dswarm, int64_t out[3]);
int hdsm_dswarm_last_path_ms(void* dswarm, float* ms);

/* ---- map updates in flight (ABI 1.7): the device world edited box by box between two rounds ------------------------------------------
 * Opt-in: a flight that calls none of these is launch for launch what it was. Boxes are lo[3] .. lo + bdim[3] in world voxels (x y z),
 * values [bdim[2]][bdim[1]][bdim[0]]; a box not inside the world, a dswarm without a world: HDSM_ERR_BAD_ARG; an empty box: a no-op.
 *   hdsm_dswarm_update_world      PROCESSED values (host pointer; synchronises, like hdsm_dswarm_set_goals) into the device world.
 *                                 The resident raw grid, if any, is not touched: the two then disagree inside the box, and a later
 *                                 raw update whose W meets it writes W from the raw grid again, over those values. Use one kind of
 *                                 update per dswarm, or repeat the processed edit after raw ones.
 *   hdsm_dswarm_set_raw_world     uploads a RAW grid of the world's dimensions (-1 unknown, 0 free, 100 occupied) and keeps it on the
 *                                 device with the scratch of the region pre-processing (4 bytes per world voxel), runs
 *                                 hdsm_map_preprocess_device on it into the device world and drops every cache entry. Synchronises,
 *                                 and reads the whole grid once on the host to check its values (a set-up call, not one for between
 *                                 two rounds). Bad arguments are refused before anything is touched; after HDSM_ERR_DEVICE the
 *                                 device world is undefined, no raw world is resident and the cache is empty.
 *   hdsm_dswarm_update_world_raw  RAW values (host pointer; synchronises) into the resident raw grid, then
 *                                 hdsm_map_preprocess_region_device into the device world: the world is then hdsm_map_preprocess
 *                                 of the edited raw grid, bit for bit. An error before hdsm_dswarm_set_raw_world.
 *   hdsm_dswarm_update_world_raw_device  the same with a device pointer, asynchronous on hip_stream. It MUST be the stream the rounds
 *                                 run on: the edit is then ordered between two rounds (the values are read when the stream gets
 *                                 there: keep them alive and unchanged until then). On another stream the edit races with a round.
 * The corridor's polyhedron cache: every update drops the entries whose decomposition could have looked at a written voxel (the
 * seed's voxel +- wave_map_radius(n_it_decomp) + 1 meets the written box — the box itself, or W of hdsm_map_region_extent for a raw
 * update; k_cache_invalidate, one lane per agent and entry); the others stay, and the slot of a dropped entry is the first to be used again. Polyhedra an agent KEEPS (AC:1253-1282) are not checked
 * against the new voxels, as in the reference and in the host mirror. Global paths adapt only through the path step (its period,
 * hdsm_dswarm_set_goals), as in the reference: an edit plans nothing by itself.
 * Several ranks: every rank holds its own copy of the world; the caller applies the same edit on every rank between the same two
 * rounds — nothing here communicates.
 *   hdsm_dswarm_download_world    synchronises and copies the processed device world out ([wdim[2]][wdim[1]][wdim[0]]), e.g. into
 *                                 hdsm_swarm_set_world of the mirror before a takeover.
 *   hdsm_dswarm_world_stats       out[0] updates applied, out[1] voxels written by them (the box, or W, summed), out[2] cache entries
 *                                 dropped (hdsm_dswarm_set_raw_world's included), out[3] 1 if a raw world is resident. Synchronises
 *                                 the device once an update has been applied (out[2] is counted there). */
int hdsm_dswarm_update_world(void* dswarm, const int8_t* values, const int32_t lo[3], const int32_t bdim[3]);
int hdsm_dswarm_set_raw_world(void* dswarm, const hdsm_map_config* map_cfg, const int8_t* raw_full);
int hdsm_dswarm_update_world_raw(void* dswarm, const int8_t* raw_values, const int32_t lo[3], const int32_t bdim[3]);
int hdsm_dswarm_update_world_raw_device(void* dswarm, const int8_t* d_raw_values, const int32_t lo[3], const int32_t bdim[3], void* hip_stream);
int hdsm_dswarm_download_world(void* dswarm, int8_t* world);
int hdsm_dswarm_world_stats(void* dswarm, int64_t out[4]);

/* ---- the flight audit (ABI 1.6): separation, obstacle contact and state history of what was flown ------------------------------
 * Opt-in; with the audit and the history off nothing is launched, allocated or written. One definition (csrc/audit_core.h) shared by
 * the host form, the host mirror and the device loop (k_audit_pack / k_audit / k_audit_track, csrc/audit_kernels.hip):
 *   separation   q = (dx^2 + dy^2) / (2 drone_radius)^2 + dz^2 / (2 drone_z_offset)^2 of the vector between two agents, sigma = sqrt(q);
 *                q >= 1 is what the separating planes ask for (AC:1158-1170). Both agents fly their records synchronously and
 *                linearly through the sub-steps s < step_plan (plans[.][s][0:3] -> plans[.][s+1][0:3]); the minimum of q along a
 *                sub-step is taken in closed form, so the whole flown segment is covered, not only the round boundaries. An agent's
 *                sep2 is the minimum of q over sub-steps and partners (ties: the smaller sub-step, then the lower id); without a
 *                partner sep2 = DBL_MAX and partner = -1. Agents with has_plan == 0 are neither subjects nor partners (their
 *                record is the empty one and their flight report does not advance).
 *   own track    per sub-step the world voxel under the end point (>= 100 occupied, < 0 unknown, 1..99 summed into pot), whether the
 *                reference's Raycast from the start to the end point hits an occupied voxel of the world grid (crossed), the length
 *                flown, and speed = |v| of plans[.][step_plan] (what SaveStateHistory averages, AC:1994-2008). Outside the world: free.
 * hdsm_flight_audit_host / _batch: plans_all [n_rob][n_hor+1][9], has_plan [n_rob], the subjects [first, first + n_local), the
 * world int8 [wdim[2]][wdim[1]][wdim[0]] (NULL = free space; wdim, worigin, voxel_size then unused) -> out[n_local]. The batch form
 * takes host pointers and copies in and out (PCIe-inclusive); the two agree bit for bit. HDSM_ERR_BAD_ARG for radii <= 0,
 * step_plan < 1 or > n_hor, or a window outside [0, n_rob). */
typedef struct hdsm_audit_round {      /* one agent, one round */
  double  sep2;                        /* min q; DBL_MAX without a partner                      */
  int32_t partner, substep;            /* global id (-1), sub-step of the minimum               */
  int32_t occupied, unknown, crossed;  /* of this round's step_plan positions / sub-segments    */
  int32_t pot;                         /* sum of the potential values 1..99 under them          */
  double  dist, speed;
} hdsm_audit_round;

typedef struct hdsm_flight_report {    /* one agent, since the audit was first switched on      */
  int64_t rounds, positions;           /* rounds audited; positions sampled (rounds * step_plan) */
  double  sep2_min;  int32_t sep_partner, sep_substep;  int64_t sep_round; /* sep_round: index among the audited rounds, -1 none */
  int64_t close_rounds;                /* rounds with q < sep_warn^2                            */
  int64_t occupied, unknown, crossed, pot_sum;
  double  dist, speed_sum, speed_max;  /* mean speed = speed_sum / rounds (AC:1994-2008)        */
} hdsm_flight_report;

int hdsm_flight_audit_host(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan, int32_t first,
                           int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world, const int32_t wdim[3],
                           const double worigin[3], double voxel_size, hdsm_audit_round* out);
int hdsm_flight_audit_batch(int32_t device, int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan,
                            int32_t first, int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world,
                            const int32_t wdim[3], const double worigin[3], double voxel_size, hdsm_audit_round* out);
/* The host mirror. hdsm_swarm_set_audit: on / off and sep_warn (> 0; the reference value is 1.0); the flight record starts when the
 * audit is switched on for the first time and is kept from then on. hdsm_swarm_audit adds one round: call it after the gather, with
 * the records all agents published this round (radii of hdsm_params, step_plan of the configuration, the world of
 * hdsm_swarm_set_world); an error while the audit is off. hdsm_swarm_flight_report: report[n_local]; an error if the audit was
 * never switched on. hdsm_swarm_get_audit: the setting as it stands (sep_warn may be NULL) — also after hdsm_dswarm_download
 * brought back what the device loop was left with. */
int hdsm_swarm_set_audit(void* swarm, int32_t on, double sep_warn);
int hdsm_swarm_get_audit(void* swarm, int32_t* on, double* sep_warn);
int hdsm_swarm_audit(void* swarm, const double* plans_all, const uint8_t* has_plan);
int hdsm_swarm_flight_report(void* swarm, hdsm_flight_report* report);
/* The device loop. The setting and the record go into hdsm_dswarm_create and come back with hdsm_dswarm_download(swarm): a flight
 * taken over in mid-air keeps its record. The audit runs at the end of hdsm_dswarm_round (after k_commit, on several ranks after
 * the exchange) on the records of all agents. hdsm_dswarm_set_audit switches it later (synchronises), hdsm_dswarm_flight_report
 * synchronises and copies report[n_local], hdsm_dswarm_last_audit_round the last round's out[n_local] (an error while the audit is off
 * or before its first round). hdsm_dswarm_last_audit_ms: with phase timing on, the duration of the last timed round's audit
 * launches; 0 if that round launched none. hdsm_dswarm_last_phase_ms keeps its seven entries: the audit starts after [6].
 * History (state_hist_, AC:240-245): hdsm_dswarm_set_history(capacity_rounds) allocates capacity x n_local x 9 doubles on the
 * device (0: off, frees them; any call starts an empty history) and every round writes state_curr after the commit into it. When it
 * is full, recording stops and the rounds lost are counted: it never wraps. hdsm_dswarm_download_history synchronises and copies the
 * first min(recorded, max_rounds) rounds into hist [.][n_local][9] (hist may be NULL), n_rounds = rounds recorded, dropped = rounds
 * lost; with a host mirror given, every recorded round not yet delivered is appended once to each agent's planner record (stamp =
 * the mirror's (round + 1) dt step_plan, as after a host round), so hdsm_swarm_shutdown writes state_hist_<id>.csv and the velocity
 * lines for a device flight as it does for a host flight. The mirror's round count, which makes the stamps, advances by the rounds
 * delivered this way and by nothing else of a device flight: hdsm_dswarm_download does not move it (as before 1.6), so rounds flown
 * on the device without a history, or lost to a full one, leave no gap in the stamps — a host round flown afterwards is stamped as
 * the next one after the last record. */
int hdsm_dswarm_set_audit(void* dswarm, int32_t on, double sep_warn);
int hdsm_dswarm_flight_report(void* dswarm, hdsm_flight_report* report);
int hdsm_dswarm_last_audit_round(void* dswarm, hdsm_audit_round* out);
int hdsm_dswarm_last_audit_ms(void* dswarm, float* ms);
int hdsm_dswarm_set_history(void* dswarm, int32_t capacity_rounds);
int hdsm_dswarm_download_history(void* dswarm, void* swarm, double* hist, int32_t max_rounds, int32_t* n_rounds, int32_t* dropped);

/* ---- neighbour groups (ABI 1.8): many independent swarms in one flight ---------------------------------------------------------
 * The definition is hdsm_set_groups' (hdsm.h): a partition of the ids into contiguous ranges group_start[n_groups + 1], and an agent's
 * neighbours are the agents of its own range — what the ungrouped code returns when has_plan is zeroed for everybody else.
 *   hdsm_swarm_set_groups     the host mirror: group_start[n_groups] must equal the mirror's n_rob (HDSM_ERR_BAD_ARG otherwise, and for
 *                             a non-zero first entry or entries that do not increase strictly); n_groups = 0 or NULL: one group. The
 *                             host reference generation (ComputePathVelocity's neighbour term) and hdsm_swarm_audit honour it.
 *   hdsm_dswarm_create        takes the mirror's partition and sets it on the solver handle it is given (no partition: it clears the
 *                             handle's): the reference, the solver and the audit of every round are grouped, on one rank or several.
 *   hdsm_dswarm_group_report  out[n_groups] (one record for the whole swarm without a partition): the device form of a per-group flight
 *                             summary over the group's LOCAL agents (k_group_report: one wavefront per group). Synchronises.
 *                             Only integer sums, minima and maxima: the result does not depend on the order of reduction. The audit
 *                             fields are zeros and -1 while the audit was never on; with it on, a group without a pair has
 *                             sep2_min = DBL_MAX and sep_agent = -1. */
typedef struct hdsm_group_report {
  int32_t first, count, n_local;       /* the group's id range [first, first + count) and how many of them are local agents     */
  int32_t no_solution_last;            /* local agents whose last status is HDSM_NO_SOLUTION                                  */
  int64_t failed_total;                /* sum of the local agents' n_fail                                                     */
  double  dist_goal_max;               /* largest distance to the goal among them                                            */
  int64_t rounds, positions, close_rounds, occupied, unknown, crossed, pot_sum; /* rounds: max; the others: sums             */
  double  sep2_min;                    /* min of the agents' sep2_min, ties to the lower agent id; DBL_MAX without a pair     */
  int32_t sep_agent, sep_partner, sep_substep, reserved0;   /* global ids (-1 none)                                          */
  int64_t sep_round;
  double  speed_max;
} hdsm_group_report;
int hdsm_swarm_set_groups(void* swarm, int32_t n_groups, const int32_t* group_start);
int hdsm_dswarm_group_report(void* dswarm, hdsm_group_report* out);

/* ---- local ranks (ABI 1.9): a sharded swarm flown by one process ------------------------------------------------------------------
 *   hdsm_dswarm_round_ranks   one replan round of ALL `world` ranks of a local communicator group (hdsm_comm_create_local, hdsm.h):
 *                             dswarms[r] is the shard of rank r of comms[r] (created with world_size = world), hip_streams[r] its
 *                             stream (NULL entries, or a NULL array: the default stream). Asynchronous. First every rank's path step,
 *                             corridor, reference, solve and k_commit (into its send buffer), then every rank's gather
 *                             (k_gather_local: one launch that copies the `world` send buffers into the rank's plans buffer and sets
 *                             the flags from the sentinel), audit and history. Ordered by events alone: a rank records "published"
 *                             behind its k_commit and "gathered" behind its gather; a gather waits for every "published" of this
 *                             round, a k_commit for every "gathered" of the round before (until then another rank may still be reading
 *                             the send buffer). All ranks on one stream is legal. HDSM_ERR_BAD_ARG, before anything is launched, when
 *                             the comms are not the ranks 0 .. world - 1 of ONE local group of exactly `world` ranks in that order, a
 *                             dswarm appears twice, is not the block of its rank, is not on its communicator's device, or the shards
 *                             disagree about n_rob or n_hor. A group of one rank is legal (it publishes through the send buffer too).
 *                             hdsm_dswarm_last_phase_ms: [6] is the rank's gather; its wait for the other ranks is counted in [5].
 *   hdsm_dswarm_download_raw  synchronises and copies out the plans buffer [world_size * per][N+1][9] AS IT IS — the sentinel of a slot
 *                             without a plan (element 0 the quiet NaN 0x7ff8000000000000, zeros behind it) included, which
 *                             hdsm_dswarm_download replaces by 0 — and the rank's send buffer [per][N+1][9] (all zeros on a single rank
 *                             without a communicator, which publishes straight into the plans buffer). Either pointer may be NULL. */
int hdsm_dswarm_round_ranks(int32_t world, void* const* dswarms, void* const* comms, void* const* hip_streams);
int hdsm_dswarm_download_raw(void* dswarm, double* plans_all_raw, double* send_raw);

/* ---- link faults in the device loop: lossy and late broadcasts (no new ABI minor; discover by symbol) ------------------------------
 * The reference has no fault injection (com_latency is declared and never used) and uses a stale neighbour plan as it is
 * (AC:1126-1147). Here every record an agent publishes has a FATE, and a round solves against what has ARRIVED:
 *   hdsm_dswarm_set_links   fate[n_rounds][n_rob] int8 (host, copied), read cyclically: entry (q mod n_rounds, k) is the fate of the
 *                           record agent k publishes in link round q — < 0: lost for everyone; d in 0..HDSM_LINK_MAX_DELAY: it arrives
 *                           d rounds late (0 = on time). Link round 0 is the first round after the call; at the call the view is the
 *                           current plans buffer and every slot counts as delivered on time. n_rounds = 0 (or fate NULL) turns links
 *                           off. The model is PER SENDER: every receiver, on every rank, sees the same thing — a link that fails for
 *                           one receiver only cannot be expressed. Ranks of a sharded swarm each get the same call. time_aware != 0:
 *                           a record that is `age` rounds old is read advanced by min(age * step_plan, N) steps, last state held
 *                           (hdsm_set_plan_shift_device, hdsm.h); 0: as it is, the reference's actual behaviour. An entry above
 *                           HDSM_LINK_MAX_DELAY: HDSM_ERR_BAD_ARG. Synchronises. Device memory is allocated by the first call only; a
 *                           flight that never calls it allocates and launches nothing new.
 * While links are on, k_deliver runs behind the exchange of every round: it keeps the last D + 1 rounds of published records (D =
 * the largest delay of the table), and per slot takes the NEWEST record that has arrived and is newer than the one held (an older
 * record that arrives after a newer one is ignored) into the `seen` view with its flag, round and shift. The next round's reference
 * and solve read `seen` / `seen_has` as the plans of the OTHER agents; every agent's own plan stays its fresh one
 * (hdsm_set_own_plans_device). The plans buffer stays the truth: the audit, the history, hdsm_dswarm_download and the takeover read it
 * unchanged — the audit judges what was flown, not what was believed.
 *   hdsm_dswarm_link_stats     out[0] link rounds since the last hdsm_dswarm_set_links, out[1] records delivered into views, out[2]
 *                              broadcasts lost, out[3] the largest age in rounds any agent's slot reached; folded on the host from the
 *                              per-slot counters. Synchronises.
 *   hdsm_dswarm_download_seen  the view as the next round reads it: seen_raw [world_size * per][N+1][9] (raw: a slot without a plan
 *                              carries the sentinel), seen_has, seen_round (link round of the record held, -1 = the view of the call)
 *                              and shift, [world_size * per] each; any pointer may be NULL. HDSM_ERR_BAD_ARG before the first
 *                              hdsm_dswarm_set_links. Synchronises.
 *   hdsm_link_deliver_host     k_deliver's round on host arrays, the same source (csrc/link_core.h), bit for bit: n_slots records
 *                              truth[n_slots][N+1][9] published in link round `link_round`; ring [max_delay + 1][n_slots][N+1][9], seen,
 *                              seen_has, seen_round, shift and counters [n_slots][4] (delivered, lost, largest age, rounds) are updated
 *                              in place. Slots k >= n_rob (padding) are delivered on time. Pure: no device, no state of its own.   */
#define HDSM_LINK_MAX_DELAY 7
int hdsm_dswarm_set_links(void* dswarm, int32_t n_rounds, const int8_t* fate, int32_t time_aware);
int hdsm_dswarm_link_stats(void* dswarm, int64_t out[4]);
int hdsm_dswarm_download_seen(void* dswarm, double* seen_raw, uint8_t* seen_has, int32_t* seen_round, int32_t* shift);
int hdsm_link_deliver_host(int32_t n_slots, int32_t n_rob, int32_t n_hor, int32_t step_plan, int32_t n_rounds, const int8_t* fate,
                           int32_t max_delay, int32_t time_aware, int32_t link_round, const double* truth, double* ring, double* seen,
                           uint8_t* seen_has, int32_t* seen_round, int32_t* shift, int32_t* counters);

/* ---- scripted agents in the device loop: movers and dropouts (no new ABI minor; discover by symbol) ------------------------------------
 * At the solver's boundary a neighbour need not be a flown agent: any record of plans_all gets a separating plane, as whoever
 * publishes on agent_<id>/traj_full does in the reference (AC:1113-1206). A SCRIPTED agent of the device loop is not planned for: it
 * follows a track and publishes the record the track gives (csrc/script_core.h, one source for the host form and k_script).
 *   track    n_knots >= 1 knots (t, x, y, z), t in seconds, finite and strictly increasing. S(tau) = (p, v, a): p_0 at rest for
 *            tau <= t_0, p_last at rest for tau >= t_last, else on the segment t_j <= tau < t_{j+1}: w = (p_{j+1} - p_j) / (t_{j+1} - t_j),
 *            p = p_j + (tau - t_j) w, v = w, a = 0 (at a knot the right-hand segment's slope).
 *   record   in script round q (0 = the first round after the call) state i of the N + 1 has the time tau_i = (double)(q * step_plan + i)
 *            * dt; tau = 0 is the start of the next round. predict = 0: states[i] = S(tau_i), the prediction is the truth.
 *            predict = 1: S(tau_i) up to i = step_plan, then the state of i = step_plan continued at constant velocity
 *            (p + ((double)(i - step_plan) * dt) v, v, a = 0) — what an observer without the track would broadcast. Either way the
 *            first step_plan segments are the true motion, which is what the flight audit judges.
 *   which    the LAST n_script ids of the shard's block. No kernel is re-indexed for it: the path step, the corridor, the reference
 *            and the solve run on the n_local - n_script agents in front of them, k_commit pads the tail's slots, and k_script — one
 *            wavefront per scripted agent, right behind k_commit on the same stream, inside entry [5] of the phase timing —
 *            overwrites exactly those slots: of the plans buffer and the flags on a single rank without a local communicator, of the
 *            send buffer otherwise (before the "published" event or the all-gather). It also writes the agent's traj_curr,
 *            state_curr = states[step_plan], has_traj = 1, the status HDSM_OK and the goal (the last knot), so the history,
 *            hdsm_dswarm_download, the audit (scripted agents are subjects and partners) and hdsm_dswarm_group_report need nothing
 *            of their own. Everything behind the publish point treats the record like any other: the exchange and k_gather_local move
 *            it, k_deliver applies its fate (a lost broadcast of a mover is a missed observation). Neighbour groups: a scripted
 *            agent is a neighbour of the range that covers its id — with a partition on one rank only the last ranges can hold
 *            movers; with local ranks every rank's block has a tail of its own. n_script = n_local is legal: the rank solves
 *            nothing. The ellipsoid is hdsm_params' for everyone.
 *   hdsm_dswarm_set_script    knots [n_script][n_knots][4] (host, copied). Synchronises, like hdsm_dswarm_set_goals. n_script may stay
 *                             (the tracks are replaced, tau starts at 0 again) or grow — the dropout: the last agents stop being
 *                             flown and go where their tracks say from the next round on. HDSM_ERR_BAD_ARG, before anything is
 *                             touched: a shrinking n_script (a scripted agent has no planner state to resume from), n_script >
 *                             n_local, n_knots outside 1..256, times that do not increase, a non-finite entry, predict outside {0, 1}.
 *                             n_script = 0 on an unscripted dswarm is a no-op. Device memory is allocated by the first call that
 *                             scripts somebody; a flight that never calls it allocates and launches nothing new. Scripting is NOT
 *                             carried into the host mirror by hdsm_dswarm_download (the mirror receives the scripted agents' states as
 *                             they stand and would plan for them): after a takeover the caller sets the script again.
 *   hdsm_dswarm_script_stats  out[0] script rounds since the last hdsm_dswarm_set_script, out[1] n_script, out[2] launches of k_script
 *                             since hdsm_dswarm_create. Host counters: it does not synchronise.
 *   hdsm_script_records_host  the records [n_script][n_hor + 1][9] of script round `round` (0 .. 2^40), pure: no device, no state.
 *   hdsm_script_records_batch the same through k_script on `device` (host pointers, copied in and out); the two agree bit for bit.
 *                             Both: HDSM_ERR_BAD_ARG for the track refusals above, n_hor outside 1..HDSM_MAX_HOR, step_plan outside
 *                             1..n_hor, dt not positive and finite. */
int hdsm_dswarm_set_script(void* dswarm, int32_t n_script, int32_t n_knots, const double* knots, int32_t predict);
int hdsm_dswarm_script_stats(void* dswarm, int64_t out[3]);
int hdsm_script_records_host(int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan, double dt,
                             int32_t predict, int64_t round, double* records);
int hdsm_script_records_batch(int32_t device, int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan,
                              double dt, int32_t predict, int64_t round, double* records);

/* ---- imperfect tracking: disturbed and measured states in the loop (no new ABI minor; discover by symbol) --------------------------------
 * The loop is closed on the reference's assumption that the vehicle arrives where its plan said: after every commit state_curr =
 * traj_curr[step_plan] (AC:233-238). Two ways to fly something else, both opt-in (csrc/track_core.h, one source for the host forms and
 * k_track): a disturbance MODEL applied right behind every commit, and a state taken from OUTSIDE (a simulator, odometry) between two
 * rounds. The published record is never touched: an agent broadcasts its plan before it flies it, so the records, and with them the
 * device audit, stay what was INTENDED; what was FLOWN is in state_curr, the state history and the next round's corridor,
 * reference and x_0.
 *   draws    a counter hash, no state and no libm. mix(z), uint64 with wrap-around: z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31). h = mix(mix(mix(seed ^ 0x9E3779B97F4A7C15) + id) + q), id the
 *            agent's GLOBAL id, q the tracking round (0 = the first round after hdsm_*_set_tracking; it restarts at every call).
 *            Draw c of 0..5: s_c = 2.0 * ((double)(mix(h + c + 1) >> 11) * 0x1p-53) - 1.0, in [-1, 1), every step exact. Keyed by the
 *            global id, a sharded flight draws what the one-rank flight draws.
 *   model    x = traj_curr[step_plan] = (p, v, a), T = (double)step_plan * dt. Per axis: w = wind + gust * s_ax; tw = T * w;
 *            p' = (p + 0.5 * (T * tw)) + jitter * s_{3+ax}; v' = v + tw; a' = a — a disturbance acceleration held over the flown
 *            interval plus a position jitter. No memory: the vehicle's own controller is taken to recover the plan up to this
 *            round's disturbance, also after a shift-by-one fallback. wind, gust in m/s^2, jitter in m; gust and jitter are
 *            amplitudes >= 0; every entry finite.
 *   record   per agent (hdsm_track_record): d = sqrt(dx*dx + dy*dy + dz*dz) of the stored p' - p and the same norm of v' - v.
 *            A model round: rounds += 1; a state taken from outside: external += 1, d and the velocity norm against the state it
 *            replaces. Both: dist_sum += d, dist_sq_sum += d*d, dist_max and dvel_max by comparison — over rounds + external samples
 *            the sum, the sum of squares and the maximum that planner_crazyswarm_bridge/scripts/tracking_error.py reports.
 *   who      an agent without a plan (has_traj == 0) has nothing to deviate from: the model leaves it alone and does not count it.
 *            Scripted agents are never touched, by the model or from outside: their state is the track's.
 *   hdsm_track_states_host    flown [n][9] (and dist [n], or NULL) of the n agents agent_id (global ids) in tracking round `round` from
 *                             planned [n][9] and the flown interval T = step_plan * dt; pure. hdsm_track_states_batch: the same through
 *                             k_track on `device` (host pointers), bit for bit. HDSM_ERR_BAD_ARG before anything is touched: a NULL
 *                             where a pointer is needed, a non-finite model entry, a negative gust or jitter, n < 0, T not positive
 *                             and finite, round outside 0..2^40.
 *   hdsm_swarm_set_tracking   the host mirror: hdsm_swarm_commit applies the model behind commit_one (the state history of the planner
 *                             records holds flown states). NULL switches it off and keeps the records.
 *   hdsm_swarm_set_states     states [n_local][9] from outside, mask [n_local] (NULL: all): a masked row whose nine values are finite
 *                             replaces state_curr; a row with a non-finite value is skipped and counted nowhere.
 *   hdsm_dswarm_set_tracking  the device loop: k_track, one lane per flown agent, right behind k_commit and in front of k_script, inside
 *                             entry [5] of the phase timing and before the history row is taken. Synchronises, like
 *                             hdsm_dswarm_set_script. NULL: off, records kept. Device memory for the records is allocated by the first
 *                             call that needs it; a flight that never calls any of these allocates and launches nothing new.
 *   hdsm_dswarm_set_states    host pointers; synchronises. hdsm_dswarm_set_states_device: device pointers, asynchronous on hip_stream,
 *                             which MUST be the stream the rounds run on (as for hdsm_dswarm_update_world_raw_device); keep the arrays
 *                             alive until the stream has passed the call. It applies between two rounds: the next round's corridor,
 *                             reference and x_0 see it, and while the history is on the agent's entry of the row the last round
 *                             left takes the state too (a row hdsm_dswarm_download_history has already handed to the mirror stays).
 *   hdsm_dswarm_track_stats   out[0] tracking rounds since the model was set, out[1] model launches of k_track, out[2] external
 *                             launches, both since hdsm_dswarm_create. Host counters: it does not synchronise.
 *   hdsm_dswarm_plans_device  the device addresses of the plans buffer [world * per][N + 1][9] and its flags [world * per]: read-only
 *                             for the caller, valid for the dswarm's life. With them a simulator on the same GPU reads what to execute
 *                             without a download (on the rounds' stream, or after synchronising with it).
 * The model is carried neither from the mirror into a new dswarm nor back by hdsm_dswarm_download, and neither are the track
 * records; the states travel with the agents as they do now. The caller sets the model on both sides. */
typedef struct hdsm_tracking {
  uint64_t seed;
  double wind[3], gust[3], jitter[3];
} hdsm_tracking;

typedef struct hdsm_track_record {
  int64_t rounds;    /* model rounds counted for this agent */
  int64_t external;  /* states taken from outside */
  double dist_sum, dist_sq_sum, dist_max; /* over rounds + external samples */
  double dvel_max;
} hdsm_track_record;

int hdsm_track_states_host(const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T, int64_t round,
                           double* flown, double* dist);
int hdsm_track_states_batch(int32_t device, const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T,
                            int64_t round, double* flown, double* dist);
int hdsm_swarm_set_tracking(void* swarm, const hdsm_tracking* m);
int hdsm_swarm_set_states(void* swarm, const double* states, const uint8_t* mask);
int hdsm_swarm_track_records(void* swarm, hdsm_track_record* out);
int hdsm_dswarm_set_tracking(void* dswarm, const hdsm_tracking* m);
int hdsm_dswarm_set_states(void* dswarm, const double* states, const uint8_t* mask);
int hdsm_dswarm_set_states_device(void* dswarm, const double* d_states, const uint8_t* d_mask, void* hip_stream);
int hdsm_dswarm_track_records(void* dswarm, hdsm_track_record* out);
int hdsm_dswarm_track_stats(void* dswarm, int64_t out[3]);
int hdsm_dswarm_plans_device(void* dswarm, void** d_plans, void** d_has);

/* ---- commands for the vehicle: yaw, attitude, full-state setpoints (no new ABI minor; discover by symbol) ------------------------------
 * The last step of Agent::TrajPlanningIteration: ComputeYawAngle after the solve (AC:177, 1025-1050), the yaw in the trajectory
 * message (Trajectory.msg field 11, AC:653), the attitude broadcast (ComputeAttitude, AC:1052-1069, through AC:797), and what the
 * reference's only consumer of a plan, planner_crazyswarm_bridge, makes of states[1]: a full-state command. Opt-in; one source
 * (csrc/command_core.h) for the host form, the host mirror and k_command, which agree bit for bit: atan2 and sincos are built there
 * from + - * / alone (host libm and the device's math library differ in the last bit; their error against the true functions is in
 * DESIGN §8, sincos pinned for |x| <= 1e4, NaN for |x| >= 2^20).
 *   yaw step  v = traj_ref[yaw_idx][0:3] - state_curr[0:3] with state_curr of BEFORE the commit and this round's reference. Only if
 *             n_ref > yaw_idx, v is finite and (vx vx + vy vy) + vz vz > 0.1: yaw_ref = atan2(vy, vx); err = yaw_ref - yaw, wrapped once
 *             (err > pi: err - 2 pi; err < -pi: err + 2 pi, pi = M_PI); yaw = yaw + (k_p_yaw err) dt — dt, not step_plan dt, as the
 *             reference. Otherwise the yaw stays.
 *   attitude  t = a - g, g = (0, 0, -9.81) (the mass cancels); z_b = t / sqrt(t.t) if t.t > 0, else t; x_i = (cos yaw, sin yaw, 0);
 *             y_b = z_b x x_i; x_b = y_b x z_b, neither normalised (as the reference); the matrix of the columns x_b, y_b, z_b goes
 *             through Eigen's matrix-to-quaternion rule: T = m00 + m11 + m22 > 0: s = sqrt(T + 1), w = s / 2, s = 0.5 / s, x = (m21 -
 *             m12) s, y = (m02 - m20) s, z = (m10 - m01) s; else i the largest diagonal entry (i = 0; m11 > m00: 1; m22 > m_ii: 2),
 *             j = (i + 1) % 3, k = (j + 1) % 3, s = sqrt(m_ii - m_jj - m_kk + 1), q_i = s / 2, s = 0.5 / s, w = (m_kj - m_jk) s,
 *             q_j = (m_ji + m_ij) s, q_k = (m_ki + m_ik) s. quat = (x, y, z, w), the order of geometry_msgs.
 *   records   per round and flown agent, hdsm_command each:
 *             setpoint [n_local][step_plan]: entry j is knot j + 1 of the record the agent published this round — the interval about
 *               to be flown; entry 0 is the bridge's states[1]. Its quaternion is that knot's acceleration and the yaw AFTER this
 *               round's step.
 *             pose [n_local]: the state the round ends in — state_curr after the commit, after the tracking model when one is on
 *               — with the attitude of that state. (The reference's transform carries traj_curr_[0] as translation, AC:779, one
 *               round behind its own rotation; here both are state_curr.)
 *             valid: 1 solved this round; 2 the shifted fallback of a failed solve; 0 no plan yet — pos = state_curr, vel = acc = 0 in
 *               the setpoints and the pose, like the bridge's position command before the first trajectory — or a state, yaw or
 *               quaternion that is not finite: every other field is then zero. The scripted tail's slots are zeros.
 *   hdsm_command_host         n agents on plain arrays: yaw [n] in and out; n_ref [n] and ref_point [n][3] = traj_ref[yaw_idx][0:3];
 *                             state_before [n][9]; records [n][n_hor + 1][9]; valid_in [n] (0, 1, 2); state_after [n][9] -> setpoint
 *                             [n][step_plan], pose [n] (either may be NULL), stats[2] (may be NULL) += steps taken, steps skipped.
 *                             Pure. hdsm_command_batch: the same through k_command on `device` (host pointers), bit for bit.
 *                             HDSM_ERR_BAD_ARG before anything is touched: a NULL where a pointer is needed, n < 0, n_hor outside
 *                             1..HDSM_MAX_HOR, step_plan outside 1..n_hor, yaw_idx outside 0..n_hor, dt not positive and finite, k_p_yaw
 *                             or a yaw not finite, a valid_in outside 0..2.
 *   hdsm_swarm_set_commands   the host mirror: hdsm_swarm_commit applies the round (behind the tracking model) to a yaw state of its
 *                             own — hdsm_swarm_yaw and its state stay what they are. on = 0: off, the yaw kept. yaw0 [n_local] or NULL:
 *                             zeros; given with on = 0 it is ignored. HDSM_ERR_BAD_ARG: yaw_idx outside 0..n_hor, k_p_yaw or a yaw0
 *                             not finite. hdsm_swarm_commands: the last commit's setpoint [n_local][step_plan], pose [n_local], yaw
 *                             [n_local] (any may be NULL); an error before the first hdsm_swarm_set_commands.
 *   hdsm_dswarm_set_commands  the device loop: k_command, one lane per local agent, behind k_commit, k_track and k_script, inside entry
 *                             [5] of the phase timing — ONE launch: it reads state_curr of before the commit from the solver's x_0 input
 *                             and this round's reference from the reference buffer, both still standing behind k_commit, and the
 *                             committed agent for the rest. Synchronises, like hdsm_dswarm_set_tracking. Device memory (the yaw, the
 *                             two record arrays, two counters) is allocated by the first call with on != 0; a flight that never
 *                             calls it allocates and launches nothing new, and commands never steer: plans and history are the same
 *                             with them on. Local ranks: every rank writes its own shard's commands.
 *   hdsm_dswarm_commands      synchronises and copies setpoint [n_local][step_plan], pose [n_local] (either may be NULL).
 *   hdsm_dswarm_commands_device  the device addresses of the two arrays, valid until hdsm_dswarm_destroy, written on the rounds'
 *                             stream: a simulator on the same GPU reads them there (or after synchronising with it) and answers with
 *                             hdsm_dswarm_set_states_device — planner -> command -> vehicle model -> measured state without the host.
 *                             An error before the first hdsm_dswarm_set_commands.
 *   hdsm_dswarm_command_stats out[0] launches of k_command, out[1] agent-rounds with a yaw step taken, out[2] agent-rounds skipped (the
 *                             0.1 rule, a missing reference), since hdsm_dswarm_create. Synchronises once commands were on.
 * hdsm_dswarm_create takes the mirror's command setting and yaw over, hdsm_dswarm_download(swarm) hands them back. */
typedef struct hdsm_command {
  double  pos[3], vel[3], acc[3];
  double  quat[4];                     /* x, y, z, w */
  double  yaw;
  int32_t valid, pad;
  double  reserved0;                   /* 0; the record is 128 bytes */
} hdsm_command;

int hdsm_command_host(int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw, const int32_t* n_ref,
                      const double* ref_point, const double* state_before, const double* records, const int32_t* valid_in,
                      const double* state_after, double* yaw, hdsm_command* setpoint, hdsm_command* pose, int64_t stats[2]);
int hdsm_command_batch(int32_t device, int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw,
                       const int32_t* n_ref, const double* ref_point, const double* state_before, const double* records,
                       const int32_t* valid_in, const double* state_after, double* yaw, hdsm_command* setpoint, hdsm_command* pose,
                       int64_t stats[2]);
int hdsm_swarm_set_commands(void* swarm, int32_t on, int32_t yaw_idx, double k_p_yaw, const double* yaw0);
int hdsm_swarm_commands(void* swarm, hdsm_command* setpoint, hdsm_command* pose, double* yaw);
int hdsm_dswarm_set_commands(void* dswarm, int32_t on, int32_t yaw_idx, double k_p_yaw, const double* yaw0);
int hdsm_dswarm_commands(void* dswarm, hdsm_command* setpoint, hdsm_command* pose);
int hdsm_dswarm_commands_device(void* dswarm, void** d_setpoint, void** d_pose);
int hdsm_dswarm_command_stats(void* dswarm, int64_t out[3]);
/* the own atan2 and sincos of csrc/command_core.h on n values each (s, c: sin and cos), for whoever wants to measure them */
int hdsm_command_atan2(int32_t n, const double* y, const double* x, double* out);
int hdsm_command_sincos(int32_t n, const double* x, double* s, double* c);

/* ---- a vehicle in the loop: a quadrotor and its controller behind the commit (no new ABI minor; discover by symbol) ----------------------
 * The fourth box of planner -> command -> vehicle model -> measured state: a rigid body with thrust along its z axis, first-order
 * lags on body rates and thrust, and the position / attitude controller that sits on it. It flies the setpoints of "commands for the
 * vehicle" sub-step by sub-step and its state becomes state_curr: the next round's corridor, reference and x_0 see what was flown.
 * Opt-in; one source (csrc/vehicle_core.h: the stage order and the sum order written there ARE the definition) for the host form, the
 * host mirror and k_vehicle, which agree bit for bit: only + - * / and sqrt, contraction off, sincos from csrc/command_core.h, draws
 * from csrc/track_core.h. g = (0, 0, -9.81), command_core.h's constant.
 *   settings   hdsm_vehicle, one for all agents. n_sub 1..1000 sub-steps per plan interval, h = dt / (double)n_sub. feed 0 HOLD:
 *              setpoint j is held over interval j (the bridge: states[1], once per iteration); 1 ALONG: the knot interval j starts
 *              from, advanced at constant acceleration: t = (double)s * h for sub-step s, p_r = (p_j + v_j t) + 0.5 (a_j (t t)),
 *              v_r = v_j + a_j t, a_r = a_j; knot 0 is traj_curr[0] (`start`), knot j > 0 is setpoint j - 1. acc_from 0: the
 *              acceleration written to state_curr stays the plan's (as k_track); 1: the model's acceleration at the end state.
 *              kp, kv >= 0 position and velocity gains; k_att >= 0 attitude error to body rate, 1/s; tau_rate, tau_thrust > 0 s;
 *              0 <= thrust_min <= thrust_max specific thrust, m/s^2; rate_max > 0 rad/s; drag >= 0, 1/s, world axes; seed, wind,
 *              gust (>= 0) as hdsm_tracking: w = wind + gust * s_ax with draws 0..2 under key(seed, global id, q), q the vehicle
 *              round (0 = the first round after hdsm_*_set_vehicle), drawn once per agent and round and held over it. Every entry
 *              finite; a setting that violates a bound is refused before anything is touched.
 *   state      hdsm_vehicle_state, 128 bytes: pos, vel, quat (x, y, z, w), omega (body rates), thrust, yaw_cmd (the last yaw
 *              commanded), one reserved double (0).
 *   seat       a vehicle on a 9-state (p, v, a) and a yaw: pos = p, vel = v, quat = the attitude of "commands for the vehicle" for
 *              (a, sin yaw, cos yaw) divided by its norm, omega = 0, thrust = clamp(sqrt(t.t), thrust_min, thrust_max), t = a - g,
 *              yaw_cmd = yaw.
 *   controller once per sub-step, held over it. x_b, y_b, z_b the columns of R(q); (p_r, v_r, a_r) the reference:
 *              a_c = ((a_r + kp (p_r - p)) + kv (v_r - v)) - g;  z_d = a_c / sqrt(a_c.a_c) if a_c.a_c > 0, else z_b;
 *              f_c = clamp(a_c . z_b, thrust_min, thrust_max);  x_i = (cos yaw, sin yaw, 0);  y_d = z_d x x_i divided by its norm
 *              (norm 0: y_b);  x_d = y_d x z_d;  e_R = 1/2 vee(R_d^T R - R^T R_d);  omega_c = clamp(-(k_att e_R), +-rate_max).
 *   plant      one classical RK4 step of length h over (p, v, q, omega, f) with omega_c, f_c and w held: p' = v;
 *              v' = ((f z_b(q) + g) - drag v) + w;  q' = 1/2 q (x) (0, omega);  omega' = (omega_c - omega) / tau_rate;
 *              f' = (f_c - f) / tau_thrust (evaluated as a product with 1.0 / tau, rounded once);  then q = q / sqrt(q.q).
 *   a round    step_plan * n_sub sub-steps against the step_plan setpoints of k_command. valid != 0 (2, the shifted fallback,
 *              included): flown as given, under `feed`. valid = 0 with a quaternion that is not all zero ("no plan yet"): the
 *              position held (the hold form whatever `feed` says). valid = 0 and the quaternion all zero (something upstream was not
 *              finite): the vehicle hovers where it stood at the start of the interval: p_r = p, v_r = a_r = 0, yaw = yaw_cmd.
 *              Afterwards flown[0:6] = the vehicle's position and velocity, flown[6:9] by acc_from; d and the velocity norm against
 *              planned_end (in the loop: state_curr as the commit left it, traj_curr[step_plan] for an agent with a plan) are booked
 *              as a model round of the agent's hdsm_track_record; the pose record is rewritten from the vehicle: its position,
 *              velocity, flown[6:9], ITS OWN quaternion, the commanded yaw, the last setpoint's valid. An end state that is not
 *              finite is not stored: the vehicle is re-seated on planned_end and the last yaw commanded (0 if that is not finite), the
 *              agent is counted in `reseated`, flown = planned_end, nothing is booked, dist = 0.
 *   hdsm_vehicle_default      a Crazyflie-class setting, wind and gust 0. PROPOSALS: no flight was measured with them.
 *   hdsm_vehicle_seat_host    out [n] from states [n][9] and yaw [n]; pure.
 *   hdsm_vehicle_fly_host     one round of n agents agent_id (global ids) in vehicle round `round` (0 .. 2^40): start [n][9],
 *                             setpoint [n][step_plan], planned_end [n][9], vstate [n] in and out -> flown [n][9], dist [n] and pose
 *                             [n] (either may be NULL), stats[4] (may be NULL) += agent-rounds flown, reseated, sub-steps with the
 *                             thrust clamped, sub-steps with a rate clamped. Pure. hdsm_vehicle_fly_batch: the same through
 *                             k_vehicle on `device` (host pointers), bit for bit. HDSM_ERR_BAD_ARG before anything is touched: a
 *                             NULL where a pointer is needed, a setting out of bounds, n < 0, step_plan outside 1..HDSM_MAX_HOR, dt
 *                             not positive and finite, round outside 0..2^40.
 *   hdsm_swarm_set_vehicle    the host mirror: hdsm_swarm_commit flies every agent behind the command step; the samples go into the
 *                             mirror's track records. At a switch-on (the first, and any after the vehicle was off: the agents
 *                             moved on without it) every vehicle is seated on state_curr and the command yaw; a call while it is on
 *                             changes the setting, restarts the vehicle round and keeps the vehicles. NULL: off, records kept. HDSM_ERR_BAD_ARG: a setting
 *                             out of bounds, commands off (the vehicle needs the setpoints and the yaw), a tracking model on. While a
 *                             vehicle is on, hdsm_*_set_tracking(non-NULL) and hdsm_*_set_commands(on = 0) are refused.
 *                             hdsm_*_set_states* keeps working and re-seats the masked vehicles on the given state and the agent's yaw.
 *   hdsm_dswarm_set_vehicle   the device loop: k_vehicle, one lane per flown agent, right behind k_command inside entry [5] of the
 *                             phase timing and before the history row and the audit are taken; the scripted tail is never touched.
 *                             Synchronises. Device memory (the states, four counters, the track records) is allocated by the first
 *                             call with a setting; a flight that never calls it allocates and launches nothing new.
 *   hdsm_*_vehicle_states     out [n_local]; an error before the first hdsm_*_set_vehicle. hdsm_dswarm_vehicle_states_device: the
 *                             device address, valid until hdsm_dswarm_destroy, written on the rounds' stream.
 *   hdsm_dswarm_vehicle_stats out[0] launches of k_vehicle, out[1] agent-rounds flown, out[2] reseated, out[3] sub-steps with the
 *                             thrust clamped, out[4] sub-steps with a rate clamped, since hdsm_dswarm_create. Synchronises once a
 *                             vehicle was on.
 * hdsm_dswarm_create takes the mirror's setting, vehicle round and vehicle states over, hdsm_dswarm_download(swarm) hands them back:
 * a vehicle has memory, and a flight that is taken over does not jump. */
typedef struct hdsm_vehicle {
  int32_t  n_sub, feed, acc_from, pad;
  double   kp[3], kv[3], k_att[3];
  double   tau_rate, tau_thrust, thrust_min, thrust_max;
  double   rate_max[3], drag[3];
  uint64_t seed;
  double   wind[3], gust[3];
} hdsm_vehicle;                        /* 224 bytes */

typedef struct hdsm_vehicle_state {
  double pos[3], vel[3];
  double quat[4];                      /* x, y, z, w */
  double omega[3];
  double thrust, yaw_cmd;
  double reserved0;                    /* 0; the record is 128 bytes */
} hdsm_vehicle_state;

int hdsm_vehicle_default(hdsm_vehicle* m);
int hdsm_vehicle_seat_host(const hdsm_vehicle* m, int32_t n, const double* states, const double* yaw, hdsm_vehicle_state* out);
int hdsm_vehicle_fly_host(const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt, int64_t round,
                          const double* start, const hdsm_command* setpoint, const double* planned_end, hdsm_vehicle_state* vstate,
                          double* flown, double* dist, hdsm_command* pose, int64_t stats[4]);
int hdsm_vehicle_fly_batch(int32_t device, const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt,
                           int64_t round, const double* start, const hdsm_command* setpoint, const double* planned_end,
                           hdsm_vehicle_state* vstate, double* flown, double* dist, hdsm_command* pose, int64_t stats[4]);
int hdsm_swarm_set_vehicle(void* swarm, const hdsm_vehicle* m);
int hdsm_swarm_vehicle_states(void* swarm, hdsm_vehicle_state* out);
int hdsm_dswarm_set_vehicle(void* dswarm, const hdsm_vehicle* m);
int hdsm_dswarm_vehicle_states(void* dswarm, hdsm_vehicle_state* out);
int hdsm_dswarm_vehicle_states_device(void* dswarm, void** d_states);
int hdsm_dswarm_vehicle_stats(void* dswarm, int64_t out[5]);

/* ---- missions: waypoints, arrival, stalls, fly to completion (no new ABI minor; discover by symbol) ---------------------------------------
 * What a flight is for: per agent a list of waypoints visited in order, judged on the device behind the commit. An arrival makes the next
 * waypoint the agent's goal and marks the agent due for a path at the start of the next round — no host round trip decides either.
 * Opt-in; one source (csrc/mission_core.h: the order written there IS the definition) for the host form, the host mirror and k_mission,
 * which agree bit for bit: only + - * /, sqrt and comparisons, contraction off.
 *   setting    hdsm_mission, one for all agents: n_wp 1..HDSM_MISSION_MAX_WP waypoints per agent in the table; loop 0 = done after the
 *              last waypoint, 1 = start over and count laps; dwell_rounds >= 1 consecutive rounds inside before an arrival counts;
 *              stall_rounds >= 0 (0: no stall detection); arrive_radius R > 0 m; arrive_speed V m/s (<= 0: no speed test); stall_eps
 *              >= 0 m. With it waypoints [n_local][n_wp][3] and count [n_local], 1..n_wp: the waypoints agent k visits.
 *   record     hdsm_mission_record, 128 bytes per agent: wp the current waypoint index; done; dwell; stalled (now); laps;
 *              stall_events; since (rounds since progress); arrivals (so far); done_round (-1 until done); last_arrival_round (-1
 *              before the first); dist (this round's distance to the waypoint, -1 when the state was not finite); best_dist;
 *              arrive_round[16] (mission round of the latest arrival at each waypoint, -1 before).
 *              Reset (hdsm_*_set_mission): zeros, the rounds -1, best_dist = DBL_MAX (no distance seen yet: the first round judged
 *              with a finite state counts as progress).
 *   a step     per flown agent and round, on state_curr as the round leaves it (after the commit, the tracking model and the vehicle),
 *              m the mission round (0 = the first round after hdsm_*_set_mission):
 *                1. done: nothing.
 *                2. d2 = (dx*dx + dy*dy) + dz*dz to waypoint[wp], d = sqrt(d2), v2 the same sum of the velocity.
 *                3. finite = d2 - d2 == 0 and v2 - v2 == 0; inside = finite and d2 <= R*R and (V <= 0 or v2 <= V*V).
 *                4. dist = finite ? d : -1; dwell = inside ? dwell + 1 : 0.
 *                5. dwell >= dwell_rounds, an arrival: arrive_round[wp] = last_arrival_round = m, ++arrivals, ++wp, dwell = 0; at wp ==
 *                   count: with loop wp = 0, ++laps, else done = 1, done_round = m. Unless done: the agent's goal becomes waypoint[wp],
 *                   the agent is due, best_dist = the distance from where it is to the new waypoint, since = 0, stalled = 0.
 *                6. otherwise progress is finite and d < best_dist - stall_eps: best_dist = d, since = 0, stalled = 0; without progress
 *                   ++since, and when stall_rounds > 0 and since == stall_rounds: stalled = 1, ++stall_events.
 *              Scripted agents (the shard's tail) fly no mission: their records stay as the reset left them.
 *   summary    hdsm_mission_summary of a shard: round (the mission round judged last, -1 before the first), flown agents, done,
 *              stalled now (and not done), arrivals of that round, arrivals in total, makespan (-1 until every flown agent is done, then the largest
 *              done_round). Integer sums and maxima: independent of the order of reduction.
 *   hdsm_mission_step_host    one step of n agents on plain arrays in mission round `round` (>= 0): states [n][9], waypoints
 *                             [n][n_wp][3], count [n], records [n] in and out -> goals [n][3] and due [n] (written for the agents that
 *                             arrived and are not done, left alone otherwise), summary (may be NULL). Pure.
 *                             hdsm_mission_step_batch: the same through k_mission on `device` (host pointers), bit for bit.
 *                             HDSM_ERR_BAD_ARG before anything is touched: a NULL where a pointer is needed, n < 0, round < 0, n_wp
 *                             outside 1..16, a count outside 1..n_wp, dwell_rounds < 1, stall_rounds < 0, loop not 0 or 1,
 *                             arrive_radius not positive and finite, arrive_speed or stall_eps not finite, stall_eps < 0, a waypoint
 *                             that is not finite, a record's wp outside 0..count - 1 (count itself for a record that is done).
 *   hdsm_swarm_set_mission    the host mirror: records reset, every agent's goal becomes its waypoint 0 and is due at the next round;
 *                             hdsm_swarm_commit steps the mission behind the vehicle. NULL: off; goals and records stay.
 *                             hdsm_swarm_mission_records / _summary: out [n_local] / one summary; an error before the first setting.
 *                             hdsm_swarm_mission_due: the agents due at the next path step [n_local] and every agent's goal
 *                             [n_local][3] (either may be NULL).
 *   hdsm_dswarm_set_mission   the device loop: k_mission, one lane per flown agent, the last launch of entry [5] of the phase timing,
 *                             behind k_vehicle. It writes an arrived agent's goal into the path step's goal buffer and sets its due
 *                             flag ON THE DEVICE; while a mission is on the path step is launched over the flown agents and a
 *                             workgroup whose agent is not flagged returns at once (rounds of the path period plan everybody, as
 *                             without). A set-up call: it synchronises. Device memory is allocated by the first call with a setting; a
 *                             flight that never calls it allocates and launches nothing new. NULL: off; goals and records stay, flags
 *                             still pending go to the host's list. While a mission is on hdsm_dswarm_set_goals returns
 *                             HDSM_ERR_BAD_ARG, and so does an hdsm_dswarm_set_script that would script more agents (the agents a
 *                             mission flies are fixed when it is set: script first). hdsm_dswarm_path_stats keeps its meaning:
 *                             out[2] counts the launches that planned somebody — of the device-sized ones those in which a flag
 *                             was set, counted on the device.
 *   hdsm_dswarm_mission_records / _summary   synchronise and copy; an error before the first setting.
 *   hdsm_dswarm_mission_due   synchronises; the pending due flags [n_local] and the goal buffer [n_local][3] (either may be NULL). It
 *                             reads the path step, not the mission: unlike the getters above it also answers before the first
 *                             setting and while the mission is off, with the host's list of due agents.
 *   hdsm_dswarm_mission_stats out[0] launches of k_mission, out[1] path launches sized on the device, out[2] agents those launches
 *                             planned, since hdsm_dswarm_create. Synchronises once a mission was on.
 *   hdsm_dswarm_mission_groups  one record per neighbour group (one for the whole shard without a partition) over the group's local
 *                             flown agents, by k_mission_fold, one wavefront per group: count, done, stalled, arrivals, laps min and
 *                             max (0 for an empty group), makespan (the group's; -1 until all its local flown agents are done).
 *                             Synchronises; launched there and nowhere else.
 *   hdsm_dswarm_fly           issues up to max_rounds rounds on hip_stream without the caller. After every check_every (>= 1) rounds it
 *                             copies the summary into pinned memory and waits for that copy alone. It stops when done == flown; with
 *                             stop_on_stall also when done + stalled == flown: at most check_every - 1 rounds are flown past the end.
 *                             rounds_flown and last (either may be NULL) take the rounds issued and the last summary polled.
 *                             HDSM_ERR_BAD_ARG: no mission on, world_size != 1 (ranks would have to agree on stopping), max_rounds < 0,
 *                             check_every < 1.
 * hdsm_dswarm_create takes the mirror's setting, waypoints, counts, records, mission round and pending due agents over,
 * hdsm_dswarm_download(swarm) hands them back with the device's flags merged into the mirror's due agents. */
#define HDSM_MISSION_MAX_WP 16

typedef struct hdsm_mission {
  int32_t n_wp, loop, dwell_rounds, stall_rounds;
  double  arrive_radius, arrive_speed, stall_eps;
  double  reserved0;                   /* 0; the setting is 48 bytes */
} hdsm_mission;

typedef struct hdsm_mission_record {
  int32_t wp, done, dwell, stalled;
  int32_t laps, stall_events, since, arrivals;
  int64_t done_round, last_arrival_round;
  double  dist, best_dist;
  int32_t arrive_round[HDSM_MISSION_MAX_WP];
} hdsm_mission_record;                 /* 128 bytes */

typedef struct hdsm_mission_summary {
  int64_t round;
  int32_t flown, done, stalled, arrivals;
  int64_t arrivals_total, makespan;
} hdsm_mission_summary;                /* 40 bytes */

typedef struct hdsm_mission_group {
  int32_t first, count, n_local, done;
  int32_t stalled, laps_min, laps_max, reserved0;
  int64_t arrivals, makespan;
} hdsm_mission_group;                  /* 48 bytes */

int hdsm_mission_step_host(const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints,
                           const int32_t* count, hdsm_mission_record* records, double* goals, uint8_t* due, hdsm_mission_summary* summary);
int hdsm_mission_step_batch(int32_t device, const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints,
                            const int32_t* count, hdsm_mission_record* records, double* goals, uint8_t* due, hdsm_mission_summary* summary);
int hdsm_swarm_set_mission(void* swarm, const hdsm_mission* m, const double* waypoints, const int32_t* count);
int hdsm_swarm_mission_records(void* swarm, hdsm_mission_record* out);
int hdsm_swarm_mission_summary(void* swarm, hdsm_mission_summary* out);
int hdsm_swarm_mission_due(void* swarm, uint8_t* due, double* goals);
int hdsm_dswarm_set_mission(void* dswarm, const hdsm_mission* m, const double* waypoints, const int32_t* count);
int hdsm_dswarm_mission_records(void* dswarm, hdsm_mission_record* out);
int hdsm_dswarm_mission_summary(void* dswarm, hdsm_mission_summary* out);
int hdsm_dswarm_mission_due(void* dswarm, uint8_t* due, double* goals);
int hdsm_dswarm_mission_stats(void* dswarm, int64_t out[3]);
int hdsm_dswarm_mission_groups(void* dswarm, hdsm_mission_group* out);
int hdsm_dswarm_fly(void* dswarm, void* hip_stream, int32_t max_rounds, int32_t check_every, int32_t stop_on_stall, int32_t* rounds_flown,
                    hdsm_mission_summary* last);

/* ---- formations: which agent takes which slot (no new ABI minor; discover by symbol) ---------------------------------------------
 * An exact linear assignment per neighbour group, minimising the sum of the quantised squared distances between the agents and the
 * slots they take — for synchronous straight-line motion no two paths of the optimal pairing cross. Opt-in; one source
 * (csrc/assign_core.h: the order written there IS the definition) for the host form, the host mirror and k_assign, which agree bit for
 * bit: integers only, apart from the cost.
 *   problem    one neighbour group group_start[g] .. group_start[g + 1] (the rules of hdsm_swarm_set_groups; n_groups = 0 or NULL: one
 *              group of all n). Bidders: the group's agents k with active[k] != 0 (active NULL: all), in ascending order; objects: the
 *              slots at the same indices, so the problem is square, m by m, m <= HDSM_ASSIGN_MAX. An inactive agent gets slot_of[k]
 *              = -1 and price[k] = 0, and its slot is offered to nobody.
 *   cost       d2 = (dx*dx + dy*dy) + dz*dz, contraction off; t = d2 * inv_q2 with inv_q2 = 1.0 / (quantum * quantum) formed once on
 *              the host; c = t >= 2^34 ? 2^34 : (int64)t. A NULL setting stands for the defaults: quantum 0.01 m, max_iters 0.
 *   auction    forward, Jacobi form, eps-scaling. Benefit a_ij = -c_ij * (m + 1); prices start at 0; eps0 = max(1, cmax * (m + 1) / 2)
 *              with cmax the group's largest cost (integer division). Phases run while eps > 1 and then once more at eps = 1; between
 *              phases eps = max(1, eps / 4). A phase starts with everybody unassigned and the prices kept. One iteration, for all
 *              bidders unassigned at its start, on the prices at its start: j* = argmax_j (a_ij - p_j), ties to the lowest j; w the
 *              best value over j != j* (m == 1: the best value itself); bid = p_j* + (best - w) + eps. Every object that received bids
 *              takes the highest, ties to the lowest bidder: its price becomes the bid, its previous owner is unassigned. Because eps
 *              = 1 < (m + 1) / m in the scaled units the final assignment is exactly optimal for the integer costs, and the final
 *              prices are a dual solution with 0 <= dual - primal <= m.
 *   status     per group: 0 optimal; 1 the budget of iterations ran out; 2 an active agent's position is not finite; 3 a bid reached
 *              2^52. With a status other than 0 the group's active agents get the identity (slot_of[k] = k), the prices are 0 and the
 *              cost is 0; iters, bids and phases say how far the auction came. m == 0: status 0, no assignment.
 *   budget     max_iters of the setting, 0 = the default 240 m + 256 (four times the largest count recorded,
 *              profiles/assign_iterations.json). It bounds the kernel's loop: no input makes it spin.
 *   stats      per group: first, count (the group's range), active (m), status, phases, iters, bids (bidders summed over the
 *              iterations), cost (the sum of c over the assignment).
 *   hdsm_assign_host / hdsm_assign_batch   pos and slots [n][3], active [n] or NULL -> slot_of [n], price [n] indexed by slot (may be
 *              NULL), stats [max(n_groups, 1)] (may be NULL). The batch form runs k_assign on `device` — one workgroup per group, host
 *              pointers copied in and out — and agrees with the host form bit for bit. Before anything is touched: HDSM_ERR_BAD_ARG for a
 *              needed NULL, n < 0, a bad partition, a slot that is not finite, a quantum that is not positive and finite (or whose inverse
 *              square is not), max_iters < 0; HDSM_ERR_CAPACITY for a group of more than HDSM_ASSIGN_MAX active
 *              agents.
 *   hdsm_swarm_assign / hdsm_dswarm_assign   the shard's flown agents (the scripted tail is inactive) in the shard's own neighbour
 *              groups, positions from state_curr as the last round left it; slots [n_local][3] -> slot_of [n_local], stats [groups]
 *              (either may be NULL). In the device loop the positions are read on the device: no state is downloaded, only slot_of and
 *              the stats come back; a set-up call, it synchronises. apply = 1 is exactly hdsm_*_set_goals(g) with g[k] =
 *              slots[slot_of[k]] for the assigned agents and the current goal for the others, through the same path; like it, it is
 *              refused with HDSM_ERR_BAD_ARG while a mission is on. apply = 0 is always allowed. world_size != 1: HDSM_ERR_BAD_ARG (a
 *              group's agents must all be local). Device memory is allocated by the first call; a flight that never calls it allocates
 *              and launches nothing new, and no round launches it. */
#define HDSM_ASSIGN_MAX 1024           /* active agents per group */

typedef struct hdsm_assign_setting {
  double  quantum;
  int32_t max_iters, reserved0;
} hdsm_assign_setting;                 /* 16 bytes */

typedef struct hdsm_assign_stats {
  int32_t first, count, active, status;
  int32_t phases, reserved0;
  int64_t iters, bids, cost;
} hdsm_assign_stats;                   /* 48 bytes */

int hdsm_assign_host(const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start, const double* pos,
                     const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price, hdsm_assign_stats* stats);
int hdsm_assign_batch(int32_t device, const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start,
                      const double* pos, const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price,
                      hdsm_assign_stats* stats);
int hdsm_swarm_assign(void* swarm, const hdsm_assign_setting* setting, const double* slots, int32_t apply, int32_t* slot_of,
                      hdsm_assign_stats* stats);
int hdsm_dswarm_assign(void* dswarm, const hdsm_assign_setting* setting, const double* slots, int32_t apply, int32_t* slot_of,
                       hdsm_assign_stats* stats);

/* Next row f3 (ROS-free half): every local agent keeps the records of Agent::TrajPlanningIteration — comp_time_sc_ (CPU time of
 * its corridor generation), comp_time_opt_ (the duration of the fused launch, handed in with hdsm_swarm_record_solve_ms between
 * prepare and commit; comp_time_tasc_ = 0 because the planes are generated inside that launch), comp_time_tot_,
 * comp_time_tot_wall_ and state_hist_. hdsm_swarm_shutdown = Agent::OnShutdown (AC:2446-2466) for one local agent: the CSV
 * files of hdsm_stats.h in `dir` (when save_stats) and the printed report. */
int hdsm_swarm_record_solve_ms(void* swarm, double milliseconds);
int hdsm_swarm_shutdown(void* swarm, int32_t local_index, const char* dir, int32_t save_stats, char* report, int32_t report_cap);

/* Diagnostics: current positions [n_local][3], distance to goal [n_local], failures so far. */
int hdsm_swarm_state(void* swarm, double* pos, double* dist_goal, int32_t* n_fail);

/* Agent::ComputeYawAngle (AC:1025-1051) for every local agent: the yaw follows the direction from the current position to
 * reference point `yaw_idx` (projected on the x-y plane) with a P controller, yaw += k_p_yaw * error * dt, error wrapped into
 * (-pi, pi]; nothing moves while that point is closer than sqrt(0.1) m. Call it where the reference does (AC:177): after the
 * solve, BEFORE hdsm_swarm_commit advances the state. yaw_out [n_local] = Trajectory.msg:11 of the plans published this round. */
int hdsm_swarm_yaw(void* swarm, int32_t yaw_idx, double k_p_yaw, double* yaw_out);

/* What the reference's rviz publishers show of local agent `k` (AC:679-857): traj_curr_ positions [n_traj <= N + 1][3],
 * traj_ref_curr_ positions [n_ref <= N + 1][3], path_curr_ [n_path <= pmax][3], the corridor (poly_const_vec_ rows n . x <= b with
 * the capacity of hdsm_params: poly_A [poly_hor][max_rows_static][3], poly_b, poly_rows[poly_hor]; poly_seeds_ [poly_hor][3]),
 * the current position. Any output pointer may be NULL. */
int hdsm_swarm_view(void* swarm, int32_t k, double* traj_curr, int32_t* n_traj, double* traj_ref, int32_t* n_ref, double* path, int32_t pmax,
                    int32_t* n_path, int32_t* n_poly, int32_t* poly_rows, double* poly_A, double* poly_b, double* poly_seeds, double pos[3]);

#ifdef __cplusplus
}
#endif
#endif
