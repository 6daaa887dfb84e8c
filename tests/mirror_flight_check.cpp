// mirror_flight_check.cpp — the host mirror's side of the flight in and out of the device-resident loop (csrc/swarm_host.h: the adopt
// of PathStep, Audit and Commands, Swarm::adopt_goals) on the host alone. Stand-alone; built from the mirror's sources with the address
// and undefined-behaviour sanitizers by tests/test_mirror_flight.py. No solver is linked: a stand-in that follows the reference flies
// the rounds. Every property is an assertion of this program (CHECK). Exit status 0 = all held.
//
// Mirrors of 5 agents, H = 10, in two groups of 2 and 3. A "full" one has period 3, one goal changed, clearance on in a small world,
// the audit on with two audited rounds and commands on with a non-zero yaw0; a "bare" one has none of them ever switched on. Handing a
// mirror what it holds itself must change nothing: every public getter and the exported agent bytes stay, and the rounds flown after
// it are the rounds of a twin that was left alone.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../multi_agent_pkgs_amd/csrc/hdsm_internal.h"
#include "../multi_agent_pkgs_amd/csrc/swarm_host.h"

using hdsm_mirror::as_swarm;
using hdsm_mirror::Swarm;

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

namespace {

constexpr int N_ROB = 5, N = 10, P = 4, RS = 18, STEP = 1;
const int32_t GROUPS[3] = {0, 2, 5};
const int32_t WDIM[3] = {60, 40, 12};
const double WORIGIN[3] = {-3.0, -3.0, -0.9};

template <class T>
std::string bytes_of(const std::vector<T>& v) {
  return std::string(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(T));
}

struct Flight {
  void* sw = nullptr;
  std::vector<double> plans = std::vector<double>((size_t)N_ROB * (N + 1) * 9, 0.0);
  std::vector<uint8_t> has = std::vector<uint8_t>(N_ROB, 0);
  ~Flight() { hdsm_swarm_destroy(sw); }
  Swarm& mirror() { return *as_swarm(sw); }

  // one round: prepare, a stand-in for the solver (the plan runs along the reference from the state), commit, the audit while it is on
  void round() {
    std::vector<int32_t> id(N_ROB), n_poly(N_ROB), n_rows((size_t)N_ROB * P), status(N_ROB, HDSM_OPTIMAL);
    std::vector<double> state((size_t)N_ROB * 9), ref((size_t)N_ROB * N * 6), A((size_t)N_ROB * P * RS * 3), b((size_t)N_ROB * P * RS);
    CHECK(hdsm_swarm_prepare(sw, plans.data(), has.data(), id.data(), state.data(), ref.data(), n_poly.data(), n_rows.data(), A.data(), b.data()) == HDSM_OK);
    std::vector<double> traj((size_t)N_ROB * (N + 1) * 9, 0.0), ctrl((size_t)N_ROB * N * 3, 0.0);
    std::vector<uint8_t> used((size_t)N_ROB * P, 0);
    for (int k = 0; k < N_ROB; ++k) {
      double* t = &traj[(size_t)k * (N + 1) * 9];
      for (int c = 0; c < 9; ++c) t[c] = state[(size_t)k * 9 + c];
      for (int i = 1; i <= N; ++i)
        for (int c = 0; c < 6; ++c) t[i * 9 + c] = ref[((size_t)k * N + (i - 1)) * 6 + c];
      if (n_poly[k] > 0) used[(size_t)k * P] = 1;
    }
    CHECK(hdsm_swarm_commit(sw, traj.data(), ctrl.data(), used.data(), status.data(), plans.data(), has.data()) == HDSM_OK);
    int32_t on = 0;
    CHECK(hdsm_swarm_get_audit(sw, &on, nullptr) == HDSM_OK);
    if (on) CHECK(hdsm_swarm_audit(sw, plans.data(), has.data()) == HDSM_OK);
  }

  // everything the public getters and the export hook answer, as bytes (a getter that refuses leaves its code)
  std::string snapshot() {
    std::string s;
    std::vector<hdsm_sw::AgentS> agents(N_ROB);
    int32_t n_local = 0, n_rob = 0, first = 0, wdim[3] = {0, 0, 0};
    double worigin[3] = {0, 0, 0};
    const int8_t* world = nullptr;
    CHECK(hdsm_swarm_export_state(sw, agents.data(), &n_local, &n_rob, &first, nullptr, nullptr, &world, wdim, worigin) == HDSM_OK);
    CHECK(n_local == N_ROB && n_rob == N_ROB && first == 0);
    s += bytes_of(agents);
    int32_t on = -1;
    double warn = -1;
    CHECK(hdsm_swarm_get_audit(sw, &on, &warn) == HDSM_OK);
    s += "|audit " + std::to_string(on) + " " + std::to_string(warn);
    std::vector<hdsm_flight_report> rep(N_ROB);
    std::memset(rep.data(), 0, rep.size() * sizeof rep[0]);
    s += "|report " + std::to_string(hdsm_swarm_flight_report(sw, rep.data())) + bytes_of(rep);
    std::vector<hdsm_command> setpoint((size_t)N_ROB * STEP), pose(N_ROB);
    std::memset(setpoint.data(), 0, setpoint.size() * sizeof setpoint[0]), std::memset(pose.data(), 0, pose.size() * sizeof pose[0]);
    std::vector<double> yaw(N_ROB, 0.0);
    s += "|commands " + std::to_string(hdsm_swarm_commands(sw, setpoint.data(), pose.data(), yaw.data())) + bytes_of(setpoint) + bytes_of(pose) + bytes_of(yaw);
    std::vector<double> paths((size_t)N_ROB * hdsm_sw::PATH_PTS * 3);
    std::vector<int32_t> n_path(N_ROB), codes(N_ROB);
    CHECK(hdsm_swarm_get_paths(sw, hdsm_sw::PATH_PTS, paths.data(), n_path.data()) == HDSM_OK);
    s += "|paths " + bytes_of(paths) + bytes_of(n_path);
    s += "|path_errors " + std::to_string(hdsm_swarm_path_errors(sw, codes.data())) + bytes_of(codes);
    s += "|corridor_errors " + std::to_string(hdsm_swarm_corridor_errors(sw, codes.data())) + bytes_of(codes);
    std::vector<hdsm_track_record> rec(N_ROB);
    std::memset(rec.data(), 0, rec.size() * sizeof rec[0]);
    CHECK(hdsm_swarm_track_records(sw, rec.data()) == HDSM_OK);
    s += "|track " + bytes_of(rec);
    std::vector<double> pos((size_t)N_ROB * 3), dist(N_ROB);
    std::vector<int32_t> n_fail(N_ROB);
    CHECK(hdsm_swarm_state(sw, pos.data(), dist.data(), n_fail.data()) == HDSM_OK);
    s += "|state " + bytes_of(pos) + bytes_of(dist) + bytes_of(n_fail);
    return s;
  }

  std::vector<double> goals() {
    std::vector<double> g;
    for (const hdsm_sw::AgentS& a : mirror().agents) g.insert(g.end(), {a.goal[0], a.goal[1], a.goal[2]});
    return g;
  }
};

// a small world: free but for a full-height pillar between the rows with a halo of potential round it
std::vector<int8_t> make_world() {
  std::vector<int8_t> w((size_t)WDIM[0] * WDIM[1] * WDIM[2], 0);
  for (int k = 0; k < WDIM[2]; ++k)
    for (int j = 14; j <= 18; ++j)
      for (int i = 26; i <= 30; ++i) w[((size_t)k * WDIM[1] + j) * WDIM[0] + i] = (i >= 27 && i <= 29 && j >= 15 && j <= 17) ? 100 : 60;
  return w;
}

void make(Flight& f, bool full) {
  hdsm_params prm;
  std::memset(&prm, 0, sizeof prm);
  prm.n_hor = N, prm.poly_hor = P, prm.max_rows_static = RS, prm.dt = 0.1, prm.drone_radius = 0.15, prm.drone_z_offset = 0.15;
  hdsm_swarm_config cfg;
  hdsm_swarm_default_config(&cfg);
  cfg.step_plan = STEP;
  double starts[N_ROB * 3], goals[N_ROB * 3];
  for (int k = 0; k < N_ROB; ++k) {
    starts[3 * k] = 1.0, starts[3 * k + 1] = 0.4 + 1.3 * k, starts[3 * k + 2] = 1.5;
    goals[3 * k] = 12.0, goals[3 * k + 1] = 5.6 - 1.3 * k, goals[3 * k + 2] = 1.5;
  }
  CHECK(hdsm_swarm_create(&prm, &cfg, N_ROB, 0, N_ROB, starts, goals, &f.sw) == HDSM_OK);
  CHECK(hdsm_swarm_set_groups(f.sw, 2, GROUPS) == HDSM_OK);
  if (!full) return;
  const std::vector<int8_t> world = make_world();
  CHECK(hdsm_swarm_set_world(f.sw, world.data(), WDIM, WORIGIN) == HDSM_OK);
  CHECK(hdsm_swarm_set_path_clearance(f.sw, 0.9) == HDSM_OK);
  CHECK(hdsm_swarm_set_path_period(f.sw, 3) == HDSM_OK);
  CHECK(hdsm_swarm_set_audit(f.sw, 1, 1.25) == HDSM_OK);
  const double yaw0[N_ROB] = {0.3, -0.2, 1.1, 2.5, -3.0};
  CHECK(hdsm_swarm_set_commands(f.sw, 1, 3, 2.0, yaw0) == HDSM_OK);
  f.round(), f.round();  // (two audited rounds; the path step's phase is 2 of 3)
  goals[3 * 3 + 1] += 2.0;
  CHECK(hdsm_swarm_set_goals(f.sw, goals) == HDSM_OK);  // (agent 3 is due in the next round)
}

// what hand_back does with a flight, fed with what the mirror holds (copies: a piece never aliases the struct that takes it)
void adopt_own(Flight& f) {
  Swarm& sw = f.mirror();
  const std::vector<uint8_t> due = sw.path.due;
  CHECK(sw.path.adopt(sw.path.period, sw.path.round, due) == HDSM_OK);
  sw.adopt_goals(f.goals());
  if (sw.audit.ever) CHECK(sw.audit.adopt(sw.audit.on, sw.audit.sep_warn, sw.audit.flight) == HDSM_OK);
  if (sw.cmd.ever) {
    const std::vector<double> yaw = sw.cmd.yaw;
    sw.cmd.adopt(sw.cfg.step_plan, sw.cmd.on, sw.cmd.yaw_idx, sw.cmd.k_p_yaw, yaw);
  }
}

void own_flight_changes_nothing(bool full) {
  Flight a, b;
  make(a, full), make(b, full);
  const std::string before = b.snapshot();
  CHECK(a.snapshot() == before);  // (the twins are twins)
  if (full) {
    CHECK(b.mirror().path.period == 3 && b.mirror().path.round == 2 && b.mirror().path.due[3] == 1 && b.mirror().path.dmp() != nullptr);
    CHECK(b.mirror().audit.ever && b.mirror().audit.on && b.mirror().cmd.ever && b.mirror().cmd.on);
    CHECK(b.mirror().cmd.yaw[4] != 0.0 && b.mirror().audit.flight.size() == (size_t)N_ROB);
  }
  adopt_own(b);
  CHECK(b.snapshot() == before);
  Swarm& sw = b.mirror();
  if (!full) {  // never switched on stays never switched on
    CHECK(!sw.audit.ever && !sw.audit.on && !sw.cmd.ever && !sw.cmd.on && sw.path.dmp() == nullptr && sw.path.period == 0);
    CHECK(hdsm_swarm_flight_report(b.sw, nullptr) == HDSM_ERR_BAD_ARG);
    CHECK(hdsm_swarm_commands(b.sw, nullptr, nullptr, nullptr) == HDSM_ERR_BAD_ARG);
  }
  // the refusals that remain, each before anything is touched
  CHECK(sw.path.adopt(-1, 7, std::vector<uint8_t>(N_ROB, 1)) == HDSM_ERR_BAD_ARG);
  CHECK(sw.audit.adopt(true, 0.0, std::vector<hdsm_flight_report>(N_ROB)) == HDSM_ERR_BAD_ARG);
  CHECK(sw.audit.adopt(true, -1.0, std::vector<hdsm_flight_report>(N_ROB)) == HDSM_ERR_BAD_ARG);
  CHECK(hdsm_swarm_set_path_period(b.sw, -1) == HDSM_ERR_BAD_ARG && hdsm_swarm_set_audit(b.sw, 1, 0.0) == HDSM_ERR_BAD_ARG);
  CHECK(b.snapshot() == before);
  for (int r = 0; r < 3; ++r) {  // period 3 and the due agent: the path step's phase shows within these rounds
    a.round(), b.round();
    CHECK(a.snapshot() == b.snapshot());
  }
  CHECK(a.snapshot() != before);  // (the rounds flew)
}

// a flight from a device loop that switched things on which the mirror never had: each adopt leaves its struct as the setter would
void adopt_keeps_the_invariants() {
  Flight f;
  make(f, false);
  Swarm& sw = f.mirror();
  std::vector<hdsm_flight_report> rep(N_ROB);
  std::memset(rep.data(), 0, rep.size() * sizeof rep[0]);
  CHECK(sw.audit.adopt(false, 2.0, rep) == HDSM_OK);
  int32_t on = -1;
  double warn = 0;
  CHECK(sw.audit.ever && hdsm_swarm_get_audit(f.sw, &on, &warn) == HDSM_OK && on == 0 && warn == 2.0);
  CHECK(hdsm_swarm_flight_report(f.sw, rep.data()) == HDSM_OK);  // (the record exists from the adopt on)
  const std::vector<double> yaw = {0.5, 0.25, -0.5, 1.5, 3.0};
  sw.cmd.adopt(sw.cfg.step_plan, false, 4, 1.5, yaw);
  CHECK(sw.cmd.ever && !sw.cmd.on && sw.cmd.yaw_idx == 4 && sw.cmd.k_p_yaw == 1.5);
  CHECK(sw.cmd.setpoint.size() == (size_t)N_ROB * STEP && sw.cmd.pose.size() == (size_t)N_ROB);
  std::vector<double> got(N_ROB, 0.0);
  CHECK(hdsm_swarm_commands(f.sw, nullptr, nullptr, got.data()) == HDSM_OK && got == yaw);
  CHECK(sw.path.adopt(4, 9, std::vector<uint8_t>{0, 1, 0, 0, 1}) == HDSM_OK);
  CHECK(sw.path.period == 4 && sw.path.round == 9 && sw.path.due[1] == 1 && sw.path.due[4] == 1 && sw.path.due[0] == 0);
  std::vector<double> goals = f.goals();
  goals[3 * 2] = 7.5;
  sw.adopt_goals(goals);
  CHECK(f.goals() == goals && sw.path.due[2] == 0);  // (goals a device loop already planned for: nobody becomes due)
  f.round();  // (switched off: a round books no command and audits nothing)
  CHECK(sw.cmd.stats[0] == 0 && sw.cmd.stats[1] == 0 && sw.path.round == 10);
}

}  // namespace

int main() {
  own_flight_changes_nothing(true);
  own_flight_changes_nothing(false);
  adopt_keeps_the_invariants();
  if (g_failed) return std::printf("%d checks failed\n", g_failed), 1;
  std::printf("all checks held\n");
  return 0;
}
