// swarm_flight.cpp — the host mirror's side of the flight in and out of the device-resident loop (dswarm_flight.cpp: take_over reads the
// mirror's member structs, hand_back calls the adopt of each), and the three hooks that stay C (hdsm_internal.h). Pure host C++.
#include <algorithm>
#include <cstring>

#include "hdsm_internal.h"
#include "swarm_host.h"

using namespace hdsm_mirror;

int PathStep::adopt(int period_, long long round_, const std::vector<uint8_t>& due_) {
  if (period_ < 0) return HDSM_ERR_BAD_ARG;
  period = period_, round = round_, due = due_;
  return HDSM_OK;
}

void Swarm::adopt_goals(const std::vector<double>& goals) {
  for (int k = 0; k < n_local; ++k)
    for (int c = 0; c < 3; ++c) agents[k].goal[c] = goals[3 * (size_t)k + c];
}

int Audit::adopt(bool on_, double sep_warn_, std::vector<hdsm_flight_report> flight_) {
  if (!(sep_warn_ > 0)) return HDSM_ERR_BAD_ARG;
  on = on_, ever = true, sep_warn = sep_warn_;
  flight = std::move(flight_);
  return HDSM_OK;
}

void Commands::adopt(int step_plan, bool on_, int yaw_idx_, double k_p_yaw_, const std::vector<double>& yaw_) {
  ready(yaw_.size(), step_plan);
  on = on_, yaw_idx = yaw_idx_, k_p_yaw = k_p_yaw_;
  std::copy(yaw_.begin(), yaw_.end(), yaw.begin());
}

void Vehicle::adopt(bool on_, const hdsm_vehicle& m_, long long q_, std::vector<hdsm_vehicle_state> state_) {
  on = on_, ever = true, m = m_, q = q_;
  state = std::move(state_);
}

void Mission::adopt(const hdsm_mission& m_, long long q_, std::vector<double> waypoints_, std::vector<int32_t> count_,
                    std::vector<hdsm_mission_record> rec_) {
  on = ever = true, m = m_, q = q_;
  waypoints = std::move(waypoints_), count = std::move(count_), rec = std::move(rec_);
  last = hdsm_mission_rule::tally_identity();  // the tally of the round judged last is the records'
  if (q > 0)
    for (const hdsm_mission_record& r : rec) hdsm_mission_rule::tally_add(last, r, r.last_arrival_round == q - 1);
}

extern "C" {

// the plain agent states and the configuration of a shard (hdsm_dswarm_create reads the configuration; the tests read the agents)
int hdsm_swarm_export_state(void* swarm, void* agents_out, int32_t* n_local, int32_t* n_rob, int32_t* first_id, hdsm_params* prm,
                            hdsm_swarm_config* cfg, const int8_t** world, int32_t wdim[3], double worigin[3]) {
  Swarm* sw = as_swarm(swarm);
  if (!sw) return HDSM_ERR_BAD_ARG;
  if (agents_out && sw->n_local) std::memcpy(agents_out, sw->agents.data(), sizeof(AgentS) * (size_t)sw->n_local);
  if (n_local) *n_local = sw->n_local;
  if (n_rob) *n_rob = sw->n_rob;
  if (first_id) *first_id = sw->first_id;
  if (prm) *prm = sw->prm;
  if (cfg) *cfg = sw->cfg;
  if (world) *world = sw->world.data();
  for (int k = 0; k < 3; ++k) {
    if (wdim) wdim[k] = sw->world.dim[k];
    if (worigin) worigin[k] = sw->world.origin[k];
  }
  return HDSM_OK;
}

int hdsm_swarm_import_state(void* swarm, const void* agents_in, int32_t n_local) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || !agents_in || n_local != sw->n_local) return HDSM_ERR_BAD_ARG;
  std::memcpy(sw->agents.data(), agents_in, sizeof(AgentS) * (size_t)n_local);
  return HDSM_OK;
}

// rounds flown on the device into the planner records (state_hist_, AC:240-245): rows [n_rounds][n_local][9], stamped as the
// rounds hdsm_swarm_commit books. round.idx counts the rounds with a record: it advances here and in hdsm_swarm_commit only
// (hdsm_swarm_import_state leaves it alone), so device rounds that were not recorded leave no gap in the stamps.
int hdsm_swarm_append_history(void* swarm, int32_t n_rounds, const double* rows) {
  Swarm* sw = as_swarm(swarm);
  if (!sw || n_rounds < 0 || (n_rounds && sw->n_local && !rows)) return HDSM_ERR_BAD_ARG;
  for (int r = 0; r < n_rounds; ++r) {
    const double stamp = (double)(sw->round.idx + 1) * sw->prm.dt * sw->cfg.step_plan;
    for (int k = 0; k < sw->n_local; ++k) hdsm_stats_add_state(sw->extra[k].stats, stamp, rows + ((size_t)r * sw->n_local + k) * 9, 9);
    ++sw->round.idx;
  }
  return HDSM_OK;
}

}  // extern "C"
