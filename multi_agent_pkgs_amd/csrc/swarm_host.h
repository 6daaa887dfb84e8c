// swarm_host.h — private header of the host mirror (include/hdsm_swarm.h, the hdsm_swarm_ entry points): the state of a shard on the
// host (Swarm) and what the files of the mirror share and nothing else — swarm_host.cpp (the round), swarm_router.cpp (hdsm_swarm_route),
// swarm_world.cpp (world and paths between rounds), swarm_models.cpp (audit, groups, tracking, commands, the vehicle) and swarm_flight.cpp (the
// flight in and out of the device-resident loop). dswarm_flight.cpp includes it too: take_over reads the member structs, hand_back
// gives each its piece back through that struct's adopt.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/hdsm_stats.h"
#include "../../include/hdsm_swarm.h"
#include "mission_core.h"
#include "path_core.h"
#include "swarm_core.h"

namespace hdsm_mirror __attribute__((visibility("hidden"))) {

using hdsm_sw::AgentS;
using hdsm_sw::norm;
using hdsm_sw::sub;
using hdsm_sw::V3;

// host-only companions of an agent's plain state (hdsm_sw::AgentS)
struct AgentX {
  void* stats = nullptr;         // hdsm_stats record of this agent (comp_time_*_, state_hist_; f3)
  double sc_ms = 0, ref_ms = 0;  // CPU time of this round's corridor / reference generation
  double yaw = 0;                // yaw_ (AC:16, 1025-1051)
};

// optional occupancy of the world (hdsm_swarm_set_world): voxels of cfg.voxel_size, >= 100 occupied
struct World {
  bool has = false;
  std::vector<int8_t> grid;
  int dim[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0};
  const int8_t* data() const { return has ? grid.data() : nullptr; }
};

// the path step (path_core.h; hdsm_swarm_set_path_period / hdsm_swarm_set_goals): every agent is due in rounds with
// round % period == 0 (period 0: never), an agent whose goal changed in the next round
struct PathStep {
  int period = 0;
  long long round = 0;
  std::vector<uint8_t> due;
  // the path step's clearance mode (hdsm_swarm_set_path_clearance): the tunnel's radius (0: off, the plain step) and its mask
  double clearance = 0;
  hdsm_path::DmpMask mask{};
  const hdsm_path::DmpMask* dmp() const { return clearance != 0 ? &mask : nullptr; }
  // (swarm_flight.cpp; the mirror and the device count rounds the same way) the phase and the pending agents a device loop was left with
  int adopt(int period_, long long round_, const std::vector<uint8_t>& due_);
};

// the flight audit (audit_core.h; hdsm_swarm_set_audit): the record starts when the audit is first switched on and is kept
struct Audit {
  bool on = false, ever = false;
  double sep_warn = 1.0;
  std::vector<hdsm_flight_report> flight;
  std::vector<hdsm_audit_round> last;
  // (swarm_flight.cpp) the setting and the record [n_local] a device loop was left with
  int adopt(bool on_, double sep_warn_, std::vector<hdsm_flight_report> flight_);
};

// neighbour groups (hdsm_swarm_set_groups): the partition as given (empty: none) and the id range per agent, [n_rob][2]
struct Groups {
  std::vector<int32_t> start, range;
  int n() const { return start.empty() ? 0 : (int)start.size() - 1; }
};

// imperfect tracking (track_core.h; hdsm_swarm_set_tracking / _set_states): the model while it is on, the tracking round the next
// commit flies, the record per agent (empty until the first call that needs it)
struct Track {
  bool on = false;
  hdsm_tracking model{};
  long long q = 0;
  std::vector<hdsm_track_record> rec;
  void ready(int n_local) {
    if (rec.size() != (size_t)n_local) rec.assign((size_t)n_local, hdsm_track_record{});
  }
};

// commands for the vehicle (command_core.h; hdsm_swarm_set_commands): the setting, a yaw state of its own (AgentX::yaw stays
// hdsm_swarm_yaw's), the last commit's records and the counters [steps taken, skipped]
struct Commands {
  bool on = false, ever = false;
  int yaw_idx = 0;
  double k_p_yaw = 0;
  std::vector<double> yaw;
  std::vector<hdsm_command> setpoint, pose;
  int64_t stats[2] = {0, 0};
  // the records of n agents, allocated by the first call that needs them
  void ready(size_t n, int step_plan) {
    if (ever) return;
    yaw.assign(n, 0.0);
    setpoint.assign(n * (size_t)step_plan, hdsm_command{}), pose.assign(n, hdsm_command{});
    ever = true;
  }
  // (swarm_flight.cpp) the setting as the device loop was left with it (switched on there and off again, k_p_yaw and yaw_idx are the
  // last ones given) and its yaw [n_local]
  void adopt(int step_plan, bool on_, int yaw_idx_, double k_p_yaw_, const std::vector<double>& yaw_);
};

// a vehicle in the loop (vehicle_core.h; hdsm_swarm_set_vehicle): the setting while it is on, the vehicle round the next commit flies,
// the state per agent (empty until the first setting; then seated) and the counters [agent-rounds flown, reseated, sub-steps with the
// thrust clamped, with a rate clamped]
struct Vehicle {
  bool on = false, ever = false;
  hdsm_vehicle m{};
  long long q = 0;
  std::vector<hdsm_vehicle_state> state;
  int64_t stats[4] = {0, 0, 0, 0};
  // (swarm_flight.cpp) the setting, the vehicle round and the states [n_local] a device loop was left with
  void adopt(bool on_, const hdsm_vehicle& m_, long long q_, std::vector<hdsm_vehicle_state> state_);
};

// a mission (mission_core.h; hdsm_swarm_set_mission): the setting while it is on, the mission round the next commit judges, the table
// [n_local][n_wp][3] with the counts, the record per agent (empty until the first setting) and the last round's tally
struct Mission {
  bool on = false, ever = false;
  hdsm_mission m{};
  long long q = 0;
  std::vector<double> waypoints;
  std::vector<int32_t> count;
  std::vector<hdsm_mission_record> rec;
  hdsm_mission_rule::Tally last = hdsm_mission_rule::tally_identity();
  // (swarm_flight.cpp) the setting, the mission round, the table and the records [n_local] a device loop was left with, switched on
  void adopt(const hdsm_mission& m_, long long q_, std::vector<double> waypoints_, std::vector<int32_t> count_, std::vector<hdsm_mission_record> rec_);
};

// timing of the round in flight (f3): the duration of the fused launch as reported by the caller, wall clock at prepare
struct Round {
  double solve_ms = 0;
  std::chrono::steady_clock::time_point t0{};
  long long idx = 0;
  bool corridor_done = false;  // hdsm_swarm_prepare_corridor already ran this round
};

struct Swarm {
  hdsm_params prm;
  hdsm_swarm_config cfg;
  int n_rob = 0, first_id = 0, n_local = 0;
  std::vector<AgentS> agents;
  std::vector<AgentX> extra;
  std::unique_ptr<hdsm_cd::Work> work{new hdsm_cd::Work};  // scratch of the voxel decomposition
  std::vector<uint32_t> bits = std::vector<uint32_t>(hdsm_cd::WindowGrid::WORDS);
  World world;
  Round round;
  PathStep path;
  Audit audit;
  Groups groups;
  Track track;
  Commands cmd;
  Vehicle veh;
  Mission mission;
  // the core configuration of an entry point: built once per call and passed down (the test hook is read at every call)
  hdsm_sw::Cfg core_cfg() const {
    hdsm_sw::Cfg c{};
    c.N = prm.n_hor, c.P = prm.poly_hor, c.RS = prm.max_rows_static, c.step_plan = cfg.step_plan;
    c.n_it_decomp = cfg.n_it_decomp, c.use_cvx_new = cfg.use_cvx_new, c.has_world = world.has ? 1 : 0;
    c.voxel_size = cfg.voxel_size, c.grid_z_min = cfg.grid_z_min, c.thresh_dist = cfg.thresh_dist;
    for (int k = 0; k < 3; ++k) c.grid_range[k] = cfg.grid_range[k], c.wdim[k] = world.dim[k], c.worigin[k] = world.origin[k];
    c.world = world.data();
    c.fast_walk = 1;  // the same walk as the device loop (shortcut past samples provably inside a kept polyhedron); 0 = every sample generated and tested
    if (const char* e = std::getenv("HDSM_FAST_WALK_HOST"))  // test hook (scalar twin of the device shortcut): "0" or "1", anything else is ignored
      if ((e[0] == '0' || e[0] == '1') && e[1] == 0) c.fast_walk = e[0] == '1';
    return c;
  }
  void neighbour_range(int id, int* lo, int* hi) const {
    *lo = groups.range.empty() ? 0 : groups.range[2 * (size_t)id], *hi = groups.range.empty() ? n_rob : groups.range[2 * (size_t)id + 1];
  }
  // (swarm_flight.cpp) the goals [n_local][3] a device loop was left with
  void adopt_goals(const std::vector<double>& goals);
  ~Swarm() {
    for (AgentX& a : extra) hdsm_stats_destroy(a.stats);
  }
};

inline Swarm* as_swarm(void* swarm) { return static_cast<Swarm*>(swarm); }

// (swarm_world.cpp) Agent::UpdatePath for one agent (dmp: the tunnel's mask in clearance mode, else NULL), and the path step at the
// start of a round
int replan_agent(const hdsm_sw::Cfg& cc, AgentS& ag, const hdsm_path::DmpMask* dmp);
void path_round(Swarm& sw, const hdsm_sw::Cfg& cc);
// (swarm_models.cpp) the steps of hdsm_swarm_commit behind the agents' own: the tracked state flown, and the commands from the
// states of before the commit ([n_local][9], commands_before; empty while commands are off)
void track_commit(Swarm& sw);
std::vector<double> commands_before(const Swarm& sw);
void commands_commit(Swarm& sw, const std::vector<double>& before, const int32_t* status);
// ... and, behind the commands, the vehicles flying this round's setpoints: state_curr, the track records and the poses take what they flew
void vehicle_commit(Swarm& sw);
// ... and, last, the mission judging what was flown: an arrival sets the agent's goal to its next waypoint and marks it in path.due, as a
// changed goal does
void mission_commit(Swarm& sw);

}  // namespace hdsm_mirror
