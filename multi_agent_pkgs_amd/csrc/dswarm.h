// dswarm.h — private host header of the hdsm_dswarm_ entry points: the state of a device-resident shard (DSwarm) and what the files
// of the loop share and nothing else — swarm_kernels.hip (the round), dswarm_world.hip (map updates in flight), dswarm_audit.hip (audit,
// history, groups), dswarm_flight.cpp (the flight in and out, goals) and dswarm_models.cpp (link faults, scripted agents, imperfect
// tracking, commands, the vehicle, missions) and dswarm_assign.cpp (formations). They report through ONE error text of their own (hdsm_dswarm_last_error), not through the solver's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hdsm.h"
#include "../../include/hdsm_swarm.h"
#include "audit_device.h"
#include "device_mem.h"
#include "mission_core.h"
#include "swarm_core.h"

namespace hdsm_dswarm __attribute__((visibility("hidden"))) {

using hdsm_mem::DevBuf;
using hdsm_sw::AgentS;
using hdsm_sw::Cfg;
using hdsm_sw::V3;

// (swarm_kernels.hip, next to the thread's error text)
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(HDSM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int PTS = hdsm_sw::PATH_PTS + 1;  // points of a reference polyline handed to k_reference

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

// commands for the vehicle (hdsm_dswarm_set_commands; nothing is allocated or launched before the first call that switches them on):
// the setting, the yaw per agent ([n_local], a buffer of its own: AgentS is shared with the mirror and stays as it is), the records
// k_command writes ([n_local][step_plan] and [n_local]), the counters [steps taken, skipped] and the launches
struct Commands {
  bool on = false;
  int yaw_idx = 0;
  double k_p_yaw = 0;
  long long launches = 0;
  DevBuf<double> d_yaw;
  DevBuf<hdsm_command> d_setpoint, d_pose;
  DevBuf<unsigned long long> d_cnt;
  bool ready() const { return (bool)d_cnt; }
};

// a vehicle in the loop (hdsm_dswarm_set_vehicle; nothing is allocated or launched before the first call with a setting): the setting
// while it is on, the vehicle round the next k_vehicle flies, the launches, the state per agent ([n_local]; the scripted tail's are never
// touched) and the counters [agent-rounds flown, reseated, sub-steps with the thrust clamped, with a rate clamped]
struct Vehicle {
  bool on = false;
  hdsm_vehicle m{};
  long long q = 0, launches = 0;
  DevBuf<hdsm_vehicle_state> d_state;
  DevBuf<unsigned long long> d_cnt;
  bool ready() const { return (bool)d_cnt; }
};

// a mission (hdsm_dswarm_set_mission; nothing is allocated or launched before the first call with a setting): the setting while it is
// on, the mission round the next k_mission judges, the launches, the table ([n_local][MAX_WP][3] allocated once, n_wp of them in use)
// and the counts, the record per agent, the due flags k_mission sets and the path step clears, the two tally slots of the summary,
// the device counters [agents the device-sized path launches planned, the last such launch that planned somebody, how many did], the pinned copy hdsm_dswarm_fly polls and its event
struct Mission {
  bool on = false;
  hdsm_mission m{};
  long long q = 0, launches = 0, path_launches = 0;
  DevBuf<double> d_wps;
  DevBuf<int32_t> d_count;
  DevBuf<hdsm_mission_record> d_rec;
  DevBuf<uint8_t> d_flag;
  DevBuf<hdsm_mission_rule::Tally> d_tally;
  DevBuf<unsigned long long> d_planned;
  DevBuf<hdsm_mission_group> d_groups;  // with the partition d_gstart, by the first hdsm_dswarm_mission_groups
  DevBuf<int32_t> d_gstart;
  hdsm_mem::PinnedBuf polled;
  hdsm_mem::DevEvent copied;
  bool ready() const { return (bool)d_planned; }
};

// formations (hdsm_dswarm_assign, dswarm_assign.cpp; nothing is allocated or launched before the first call, and no round launches
// it): the slots as given, the assignment and the stats per group k_assign writes, the partition (one group without one), the launches
struct Assign {
  long long launches = 0;
  DevBuf<double> d_slots;
  DevBuf<int32_t> d_slot_of, d_gstart;
  DevBuf<hdsm_assign_stats> d_stats;
  bool ready() const { return (bool)d_stats; }
};

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
  Commands cmd;
  int n_fly() const { return n_local - script.n; }  // the agents this shard plans for: all but its scripted tail
  int slots() const { return per * world; }         // the records of the plans buffer (and of everything shaped like it)
  int rec() const { return (c.N + 1) * 9; }         // the doubles of a record
  size_t voxels() const { return (size_t)c.wdim[0] * c.wdim[1] * c.wdim[2]; }  // of the world
  // where k_commit and k_script publish: one rank without a local communicator (`direct`) straight into the plans buffer, else into
  // the send buffer of the exchange
  double* publish_to(bool direct) const { return direct ? d_plans.get() : d_local.get(); }
  // neighbour groups (taken from the mirror by hdsm_dswarm_create; one group = the whole swarm without a partition): the
  // partition, the id range per record of the plans buffer ([per * world][2], for the audit; null without a partition), the report
  std::vector<int32_t> group_start;
  bool grouped = false;
  DevBuf<int32_t> d_gstart, d_range;
  DevBuf<hdsm_group_report> d_greport;
  Vehicle veh;
  Mission mission;
  Assign assign;
};

inline DSwarm* as_dswarm(void* dswarm) { return static_cast<DSwarm*>(dswarm); }

// the dswarm's device is the thread's and has nothing left to do
inline int device_idle(const DSwarm* d) {
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

// (dswarm_flight.cpp) every agent's goal and the list of the agents marked in path.due onto the device (the device is idle)
int upload_goals_and_due(DSwarm* d);
// (dswarm_flight.cpp) the mirror's flight becomes the device's, and the way back
int take_over(DSwarm& d, void* swarm, const int8_t* hworld);
int hand_back(DSwarm& d, void* swarm);
// (dswarm_models.cpp) the command buffers, allocated by the first call that needs them (the caller has set the device); the setting
// and the yaw [n_local] (NULL: zeros) onto the device (the device is idle)
int commands_setup(DSwarm* d, bool on, int yaw_idx, double k_p_yaw, const double* yaw0);
// (dswarm_models.cpp) the vehicle buffers, allocated by the first call that needs them, and the setting switched on (the caller has set
// the device, which is idle). vs [n_local]: the states to start from; NULL: every flown agent is seated on its state_curr and yaw,
// unless the vehicle is on already.
int vehicle_setup(DSwarm* d, const hdsm_vehicle& m, long long q, const hdsm_vehicle_state* vs);
// (dswarm_models.cpp) the mission buffers, allocated by the first call that needs them, and the setting switched on with its table
// (the caller has set the device, which is idle). rec [n_local] and due [n_local]: the records and pending agents to go on from, with
// the mission round q; NULL: the records are reset, every flown agent turns to its waypoint 0 and is due.
int mission_setup(DSwarm* d, const hdsm_mission& m, const double* waypoints, const int32_t* count, long long q, const hdsm_mission_record* rec,
                  const uint8_t* due);
// (dswarm_models.cpp) once a mission was set the goals live on the device: the goal buffer into path.goals (the device is idle)
int mission_pull_goals(DSwarm* d);
// (swarm_kernels.hip) every event a timed round records
int timing_events(DSwarm* d);
// (dswarm_audit.hip) the audit's scratch and (at the first switch-on) the flight record of the shard; `init` [n_local] or empty reports
int audit_setup(DSwarm* d, const hdsm_flight_report* init);

}  // namespace hdsm_dswarm
