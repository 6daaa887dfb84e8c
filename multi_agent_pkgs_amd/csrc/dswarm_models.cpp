// dswarm_models.cpp — what a caller puts between the plans and the flight of the device-resident loop, set between rounds: link faults
// (k_deliver, swarm_kernels.hip), scripted agents (k_script, script_kernels.hip), imperfect tracking (k_track, track_kernels.hip), the
// commands for the vehicle (k_command, command_kernels.hip), the vehicle itself (k_vehicle, vehicle_kernels.hip) and missions (k_mission,
// mission_kernels.hip, with hdsm_dswarm_fly), each with its counters and downloads. Semantics in include/hdsm_swarm.h. The only launches
// from here are k_track's external form (hdsm_dswarm_set_states*, through track_device.h), k_seat (a vehicle seated at a switch-on or
// on a state from outside, through vehicle_device.h) and k_mission_fold (hdsm_dswarm_mission_groups, through mission_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "command_core.h"
#include "dswarm.h"
#include "link_core.h"
#include "mission_device.h"
#include "script_device.h"
#include "track_device.h"
#include "vehicle_device.h"

using namespace hdsm_dswarm;

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
    // a vehicle that sits on the agent is re-seated on what was measured (the same rows: masked and finite), with the agent's yaw
    if (d->veh.ready())
      HIP_TRY(hdsm_veh::launch_seat(hdsm_veh::Seat{n_fly, d->veh.m, d_states, 9, d->cmd.d_yaw.get(), d_mask, d->veh.d_state.get()}, st));
  }
  return HDSM_OK;
}

}  // namespace

int hdsm_dswarm::commands_setup(DSwarm* d, bool on, int yaw_idx, double k_p_yaw, const double* yaw0) {
  Commands& m = d->cmd;
  const size_t n = (size_t)d->n_local;
  if (on && !m.ready()) {
    hdsm_mem::FirstError ok;
    ok(m.d_yaw.alloc_zeroed(n)), ok(m.d_setpoint.alloc_zeroed(n * (size_t)d->c.step_plan)), ok(m.d_pose.alloc_zeroed(n)), ok(m.d_cnt.alloc_zeroed(2));
    if (!ok.ok()) {
      m.d_cnt.reset();
      return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_set_commands: ") + hipGetErrorString(ok.e));
    }
  }
  if (on) {
    if (yaw0 && n) HIP_TRY(hipMemcpy(m.d_yaw.get(), yaw0, n * sizeof(double), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(m.d_yaw.get(), 0, (n ? n : 1) * sizeof(double)));
    HIP_TRY(hipDeviceSynchronize());  // (the fills are done before a kernel of any stream writes into the buffers)
    m.yaw_idx = yaw_idx, m.k_p_yaw = k_p_yaw;
  }
  m.on = on;
  return HDSM_OK;
}

int hdsm_dswarm::vehicle_setup(DSwarm* d, const hdsm_vehicle& m, long long q, const hdsm_vehicle_state* vs) {
  Vehicle& v = d->veh;
  const size_t n = (size_t)d->n_local;
  if (int rc = track_records_ready(d)) return rc;
  const bool first = !v.ready();
  if (first) {
    hdsm_mem::FirstError ok;
    ok(v.d_state.alloc_zeroed(n)), ok(v.d_cnt.alloc_zeroed(4));
    if (!ok.ok()) {
      v.d_cnt.reset();
      return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_set_vehicle: ") + hipGetErrorString(ok.e));
    }
    HIP_TRY(hipDeviceSynchronize());  // (the fills are done before a kernel of any stream writes into the buffers)
  }
  v.m = m, v.q = q;
  if (vs != nullptr) {
    if (n) HIP_TRY(hipMemcpy(v.d_state.get(), vs, n * sizeof(hdsm_vehicle_state), hipMemcpyHostToDevice));
  } else if (!v.on && d->n_fly() > 0) {  // a switch-on: the vehicle was off (or never there) while the agents moved
    HIP_TRY(hdsm_veh::launch_seat(hdsm_veh::Seat{d->n_fly(), m, &d->d_agents.get()[0].state_curr[0], sizeof(AgentS) / sizeof(double), d->cmd.d_yaw.get(),
                                                 nullptr, v.d_state.get()},
                                  nullptr));
    HIP_TRY(hipDeviceSynchronize());
  }
  v.on = true;
  return HDSM_OK;
}

int hdsm_dswarm::mission_pull_goals(DSwarm* d) {
  if (d->mission.ready() && d->n_local > 0)
    HIP_TRY(hipMemcpy(d->path.goals.data(), d->path.d_goals.get(), d->path.goals.size() * sizeof(double), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm::mission_setup(DSwarm* d, const hdsm_mission& m, const double* waypoints, const int32_t* count, long long q,
                               const hdsm_mission_record* rec, const uint8_t* due) {
  using hdsm_mission_rule::Tally;
  Mission& ms = d->mission;
  const size_t n = (size_t)d->n_local;
  const int n_fly = d->n_fly();
  if (!ms.ready()) {
    hdsm_mem::FirstError ok;
    ok(ms.d_wps.alloc(n * hdsm_mission_rule::MAX_WP * 3)), ok(ms.d_count.alloc(n)), ok(ms.d_rec.alloc_zeroed(n)), ok(ms.d_flag.alloc_zeroed(n));
    ok(ms.d_tally.alloc(2)), ok(ms.polled.ensure(2 * sizeof(Tally))), ok(ms.copied.create(hipEventDisableTiming)), ok(ms.d_planned.alloc_zeroed(3));
    if (!ok.ok()) {
      ms.d_planned.reset();
      return fail(HDSM_ERR_DEVICE, std::string("hdsm_dswarm_set_mission: ") + hipGetErrorString(ok.e));
    }
  }
  ms.on = false;
  Tally tally[2] = {hdsm_mission_rule::tally_identity(), hdsm_mission_rule::tally_identity()};
  if (n) {
    HIP_TRY(hipMemcpy(ms.d_wps.get(), waypoints, n * 3 * (size_t)m.n_wp * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ms.d_count.get(), count, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(ms.d_flag.get(), 0, n));
  }
  if (rec != nullptr) {  // a flight taken over goes on from its records; the tally of the round judged last is theirs
    if (n) HIP_TRY(hipMemcpy(ms.d_rec.get(), rec, n * sizeof(hdsm_mission_record), hipMemcpyHostToDevice));
    if (due != nullptr && n_fly > 0) HIP_TRY(hipMemcpy(ms.d_flag.get(), due, (size_t)n_fly, hipMemcpyHostToDevice));
    if (q > 0)
      for (int k = 0; k < n_fly; ++k) hdsm_mission_rule::tally_add(tally[(q - 1) & 1], rec[k], rec[k].last_arrival_round == q - 1);
  } else if (n) {  // a new mission: blank records, every flown agent turns to its waypoint 0 and is flagged for the next round's path step
    std::vector<hdsm_mission_record> blank(n);
    for (hdsm_mission_record& r : blank) hdsm_mission_rule::reset(r);
    HIP_TRY(hipMemcpy(ms.d_rec.get(), blank.data(), n * sizeof(hdsm_mission_record), hipMemcpyHostToDevice));
    if (int rc = mission_pull_goals(d)) return rc;
    for (int k = 0; k < n_fly; ++k)
      for (int c = 0; c < 3; ++c) d->path.goals[3 * (size_t)k + c] = waypoints[(size_t)k * 3 * m.n_wp + c];
    HIP_TRY(hipMemcpy(d->path.d_goals.get(), d->path.goals.data(), d->path.goals.size() * sizeof(double), hipMemcpyHostToDevice));
    if (n_fly > 0) HIP_TRY(hipMemset(ms.d_flag.get(), 1, (size_t)n_fly));
  }
  HIP_TRY(hipMemcpy(ms.d_tally.get(), tally, sizeof tally, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  // who is due is on the device from here on: the host's list is empty while the mission is on
  std::fill(d->path.due.begin(), d->path.due.end(), (uint8_t)0);
  d->path.n_due = 0;
  ms.m = m, ms.q = q, ms.on = true;
  return HDSM_OK;
}

namespace {

// the summary of the mission round judged last, from the two tally slots as they stand on the device or in the polled copy
hdsm_mission_summary mission_summary_of(const DSwarm& d, const hdsm_mission_rule::Tally* tally) {
  const long long last = d.mission.q - 1;
  // (before the first round, and on a shard that flies nobody — where k_mission is never launched and nothing resets a slot — the
  // summary is the identity's: nothing done, makespan -1)
  const bool judged = last >= 0 && d.n_fly() > 0;
  return hdsm_mission_rule::summary_of(judged ? tally[last & 1] : hdsm_mission_rule::tally_identity(), last, d.n_fly());
}

}  // namespace

extern "C" {

// Missions (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_mission(void* dswarm, const hdsm_mission* m, const double* waypoints, const int32_t* count) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  Mission& ms = d->mission;
  if (!m) {
    if (!ms.on) return HDSM_OK;
    if (int rc = device_idle(d)) return rc;
    // the goals and the agents still flagged go back to the host's side of the path step
    if (int rc = mission_pull_goals(d)) return rc;
    const int n_fly = d->n_fly();
    if (n_fly > 0) {
      HIP_TRY(hipMemcpy(d->path.due.data(), ms.d_flag.get(), (size_t)n_fly, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemset(ms.d_flag.get(), 0, (size_t)n_fly));
    }
    ms.on = false;
    return upload_goals_and_due(d);
  }
  if (!hdsm_mission_rule::setting_valid(m, d->n_local, waypoints, count))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_mission: a setting out of its bounds (include/hdsm_swarm.h), a count outside 1..n_wp or a waypoint not finite");
  if (int rc = device_idle(d)) return rc;
  return mission_setup(d, *m, waypoints, count, 0, nullptr, nullptr);
}

int hdsm_dswarm_mission_records(void* dswarm, hdsm_mission_record* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!out && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_records: null argument");
  if (!d->mission.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_records: no hdsm_dswarm_set_mission yet");
  if (int rc = device_idle(d)) return rc;
  if (d->n_local) HIP_TRY(hipMemcpy(out, d->mission.d_rec.get(), (size_t)d->n_local * sizeof(hdsm_mission_record), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_mission_summary(void* dswarm, hdsm_mission_summary* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_summary: null argument");
  if (!d->mission.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_summary: no hdsm_dswarm_set_mission yet");
  if (int rc = device_idle(d)) return rc;
  hdsm_mission_rule::Tally tally[2];
  HIP_TRY(hipMemcpy(tally, d->mission.d_tally.get(), sizeof tally, hipMemcpyDeviceToHost));
  *out = mission_summary_of(*d, tally);
  return HDSM_OK;
}

int hdsm_dswarm_mission_due(void* dswarm, uint8_t* due, double* goals) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (int rc = device_idle(d)) return rc;
  const size_t n = (size_t)d->n_local;
  if (n == 0) return HDSM_OK;
  if (due) {
    if (d->mission.on) HIP_TRY(hipMemcpy(due, d->mission.d_flag.get(), n, hipMemcpyDeviceToHost));
    else std::copy(d->path.due.begin(), d->path.due.end(), due);
  }
  if (goals) HIP_TRY(hipMemcpy(goals, d->path.d_goals.get(), n * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_mission_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->mission.launches, out[1] = d->mission.path_launches, out[2] = 0;
  if (!d->mission.ready()) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  unsigned long long planned = 0;
  HIP_TRY(hipMemcpy(&planned, d->mission.d_planned.get(), sizeof planned, hipMemcpyDeviceToHost));
  out[2] = (int64_t)planned;
  return HDSM_OK;
}

// The mission per group (one record for the whole shard without a partition): k_mission_fold over the records. Launched here and
// nowhere else: a round never pays for it.
int hdsm_dswarm_mission_groups(void* dswarm, hdsm_mission_group* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_groups: null argument");
  Mission& ms = d->mission;
  if (!ms.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_mission_groups: no hdsm_dswarm_set_mission yet");
  const int ng = (int)d->group_start.size() - 1;
  if (int rc = device_idle(d)) return rc;
  if (!ms.d_gstart) {
    HIP_TRY(ms.d_groups.alloc((size_t)ng));
    HIP_TRY(ms.d_gstart.alloc(d->group_start.size()));
    HIP_TRY(hipMemcpy(ms.d_gstart.get(), d->group_start.data(), d->group_start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(hdsm_mission_rule::launch_fold(ng, d->first, d->n_fly(), ms.d_gstart.get(), ms.d_rec.get(), ms.d_groups.get(), nullptr));
  HIP_TRY(hipMemcpy(out, ms.d_groups.get(), (size_t)ng * sizeof(hdsm_mission_group), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// Rounds without the caller: every check_every rounds the two tally slots are copied into pinned memory on the rounds' stream and the
// host waits for that copy alone — the event behind it — before it decides whether to go on.
int hdsm_dswarm_fly(void* dswarm, void* hip_stream, int32_t max_rounds, int32_t check_every, int32_t stop_on_stall, int32_t* rounds_flown,
                    hdsm_mission_summary* last) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (rounds_flown) *rounds_flown = 0;
  if (d->world != 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_fly: world_size 1 only (ranks would have to agree on stopping)");
  Mission& ms = d->mission;
  if (!ms.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_fly: no mission is on (hdsm_dswarm_set_mission)");
  if (max_rounds < 0 || check_every < 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_fly: max_rounds >= 0 and check_every >= 1");
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const hdsm_mission_rule::Tally* const polled = static_cast<const hdsm_mission_rule::Tally*>(ms.polled.get());
  int32_t rounds = 0;
  for (;;) {
    if (rounds % check_every == 0 || rounds == max_rounds) {
      HIP_TRY(hipMemcpyAsync(ms.polled.get(), ms.d_tally.get(), 2 * sizeof(hdsm_mission_rule::Tally), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipEventRecord(ms.copied.get(), st));
      HIP_TRY(hipEventSynchronize(ms.copied.get()));
      const hdsm_mission_summary s = mission_summary_of(*d, polled);
      if (last) *last = s;
      if (s.done == s.flown || (stop_on_stall && s.done + s.stalled == s.flown)) break;
    }
    if (rounds == max_rounds) break;
    if (int rc = hdsm_dswarm_round(dswarm, nullptr, hip_stream)) return rc;
    ++rounds;
    if (rounds_flown) *rounds_flown = rounds;
  }
  return HDSM_OK;
}

// Link faults (include/hdsm_swarm.h). The call starts a new link history: the view is the plans buffer as it stands (every slot
// delivered on time, held round -1, shift 0), the counters are zero, link round 0 is the next round.
int hdsm_dswarm_set_links(void* dswarm, int32_t n_rounds, const int8_t* fate, int32_t time_aware) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (n_rounds < 0) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_links: negative n_rounds");
  Links& l = d->links;
  if (int rc = device_idle(d)) return rc;
  if (n_rounds == 0 || fate == nullptr) {
    l.on = false;
    return HDSM_OK;
  }
  const int D = hdsm_link::table_max_delay(n_rounds, d->n_rob, fate);
  if (D < 0) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_links: a delay above HDSM_LINK_MAX_DELAY");
  const size_t G = (size_t)d->slots(), rec = (size_t)d->rec(), cells = (size_t)n_rounds * (size_t)d->n_rob;
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

int hdsm_dswarm_link_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!d->links.ready()) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  const size_t G = (size_t)d->slots(), have = (size_t)d->n_rob < G ? (size_t)d->n_rob : G;  // (the padded tail publishes nothing)
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
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (!d->links.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_download_seen: no hdsm_dswarm_set_links yet");
  if (int rc = device_idle(d)) return rc;
  const Links& l = d->links;
  const size_t G = (size_t)d->slots(), rec = (size_t)d->rec();
  if (G == 0) return HDSM_OK;
  if (seen_raw) HIP_TRY(hipMemcpy(seen_raw, l.d_seen.get(), G * rec * 8, hipMemcpyDeviceToHost));
  if (seen_has) HIP_TRY(hipMemcpy(seen_has, l.d_seen_has.get(), G, hipMemcpyDeviceToHost));
  if (seen_round) HIP_TRY(hipMemcpy(seen_round, l.d_seen_round.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (shift) HIP_TRY(hipMemcpy(shift, l.d_shift.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// Scripted agents (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_script(void* dswarm, int32_t n_script, int32_t n_knots, const double* knots, int32_t predict) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  Script& s = d->script;
  if (n_script < s.n) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: n_script may stay or grow (a scripted agent has no planner state to resume from)");
  if (d->mission.on && n_script > s.n)
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: a mission is on (hdsm_dswarm_set_mission): the agents it flies are fixed when it is set");
  if (n_script > d->n_local) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: more scripted agents than the shard has");
  if (predict != 0 && predict != 1) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: predict is 0 or 1");
  if (!hdsm_script::tracks_valid(n_script, n_knots, knots))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_script: 1 .. 256 knots per track, every entry finite, times strictly increasing");
  if (n_script == 0) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  if (int rc = mission_pull_goals(d)) return rc;  // (once a mission was set the goals live on the device)
  if (!s.d_knots) HIP_TRY(s.d_knots.alloc((size_t)d->n_local * hdsm_script::MAX_KNOTS * 4));
  HIP_TRY(hipMemcpy(s.d_knots.get(), knots, (size_t)n_script * n_knots * 4 * sizeof(double), hipMemcpyHostToDevice));
  // a scripted agent's goal is its last knot, and it plans no path: the flown agents that are due stay due
  PathStep& p = d->path;
  const int n_fly = d->n_local - n_script;
  for (int k = n_fly; k < d->n_local; ++k) {
    const double* last = knots + ((size_t)(k - n_fly) * n_knots + (n_knots - 1)) * 4;
    for (int q = 0; q < 3; ++q) p.goals[3 * (size_t)k + q] = last[1 + q];
    p.due[(size_t)k] = 0;
  }
  if (int rc = upload_goals_and_due(d)) return rc;
  if (d->mission.ready()) HIP_TRY(hipMemset(d->mission.d_flag.get() + n_fly, 0, (size_t)n_script));  // (a scripted agent flies no mission)
  s.n = n_script, s.n_knots = n_knots, s.predict = predict, s.round = 0;
  return HDSM_OK;
}

int hdsm_dswarm_script_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->script.round, out[1] = d->script.n, out[2] = d->script.launches;
  return HDSM_OK;
}

// Imperfect tracking (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_tracking(void* dswarm, const hdsm_tracking* m) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (m && !hdsm_track::model_valid(m))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_tracking: every entry of the model finite, gust and jitter not negative");
  if (m && d->veh.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_tracking: a vehicle is on (hdsm_dswarm_set_vehicle): it is what deviates from the plan");
  Track& t = d->track;
  if (!m && !t.on) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  if (m) {
    if (int rc = track_records_ready(d)) return rc;
    t.model = *m, t.q = 0;
  }
  t.on = m != nullptr;
  return HDSM_OK;
}

int hdsm_dswarm_set_states(void* dswarm, const double* states, const uint8_t* mask) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!states && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_states: null argument");
  if (d->n_local == 0) return HDSM_OK;
  Track& t = d->track;
  const size_t n = (size_t)d->n_local;
  if (int rc = device_idle(d)) return rc;
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
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!d_states && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_states_device: null argument");
  if (d->n_local == 0) return HDSM_OK;
  HIP_TRY(hipSetDevice(d->device));
  if (int rc = track_records_ready(d)) return rc;
  return track_external(d, d_states, d_mask, static_cast<hipStream_t>(hip_stream));
}

int hdsm_dswarm_track_records(void* dswarm, hdsm_track_record* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!out && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_track_records: null argument");
  if (d->n_local == 0) return HDSM_OK;
  if (!d->track.d_rec) {
    for (int k = 0; k < d->n_local; ++k) out[k] = hdsm_track_record{};
    return HDSM_OK;
  }
  if (int rc = device_idle(d)) return rc;
  HIP_TRY(hipMemcpy(out, d->track.d_rec.get(), (size_t)d->n_local * sizeof(hdsm_track_record), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

// Commands for the vehicle (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_commands(void* dswarm, int32_t on, int32_t yaw_idx, double k_p_yaw, const double* yaw0) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (on && !hdsm_cmd::settings_valid(yaw_idx, d->c.N, k_p_yaw, yaw0, d->n_local))
    return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_commands: yaw_idx in 0 .. n_hor, k_p_yaw and every yaw0 finite");
  if (!on && d->veh.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_commands: a vehicle is on (hdsm_dswarm_set_vehicle): it needs the setpoints and the yaw");
  if (!on && !d->cmd.on) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  return commands_setup(d, on != 0, yaw_idx, k_p_yaw, yaw0);
}

int hdsm_dswarm_commands(void* dswarm, hdsm_command* setpoint, hdsm_command* pose) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  if (!d->cmd.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_commands: no hdsm_dswarm_set_commands yet");
  if (int rc = device_idle(d)) return rc;
  const size_t n = (size_t)d->n_local;
  if (setpoint && n) HIP_TRY(hipMemcpy(setpoint, d->cmd.d_setpoint.get(), n * (size_t)d->c.step_plan * sizeof(hdsm_command), hipMemcpyDeviceToHost));
  if (pose && n) HIP_TRY(hipMemcpy(pose, d->cmd.d_pose.get(), n * sizeof(hdsm_command), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_commands_device(void* dswarm, void** d_setpoint, void** d_pose) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !d_setpoint || !d_pose) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->cmd.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_commands_device: no hdsm_dswarm_set_commands yet");
  *d_setpoint = d->cmd.d_setpoint.get(), *d_pose = d->cmd.d_pose.get();
  return HDSM_OK;
}

int hdsm_dswarm_command_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->cmd.launches, out[1] = out[2] = 0;
  if (!d->cmd.ready()) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, d->cmd.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost));
  out[1] = (int64_t)cnt[0], out[2] = (int64_t)cnt[1];
  return HDSM_OK;
}

// A vehicle in the loop (include/hdsm_swarm.h). Every refusal comes before anything is touched.
int hdsm_dswarm_set_vehicle(void* dswarm, const hdsm_vehicle* m) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d) return fail(HDSM_ERR_BAD_ARG, "null dswarm");
  Vehicle& v = d->veh;
  if (!m) {
    if (!v.on) return HDSM_OK;
    if (int rc = device_idle(d)) return rc;
    v.on = false;
    return HDSM_OK;
  }
  if (!hdsm_veh::settings_valid(m)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_vehicle: a setting out of its bounds (include/hdsm_swarm.h), or not finite");
  if (!d->cmd.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_vehicle: commands are off (hdsm_dswarm_set_commands): the vehicle needs the setpoints and the yaw");
  if (d->track.on) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_set_vehicle: a tracking model is on (hdsm_dswarm_set_tracking)");
  if (int rc = device_idle(d)) return rc;
  return vehicle_setup(d, *m, 0, nullptr);
}

int hdsm_dswarm_vehicle_states(void* dswarm, hdsm_vehicle_state* out) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || (!out && d->n_local)) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_vehicle_states: null argument");
  if (!d->veh.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_vehicle_states: no hdsm_dswarm_set_vehicle yet");
  if (int rc = device_idle(d)) return rc;
  if (d->n_local) HIP_TRY(hipMemcpy(out, d->veh.d_state.get(), (size_t)d->n_local * sizeof(hdsm_vehicle_state), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_vehicle_states_device(void* dswarm, void** d_states) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !d_states) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->veh.ready()) return fail(HDSM_ERR_BAD_ARG, "hdsm_dswarm_vehicle_states_device: no hdsm_dswarm_set_vehicle yet");
  *d_states = d->veh.d_state.get();
  return HDSM_OK;
}

int hdsm_dswarm_vehicle_stats(void* dswarm, int64_t out[5]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->veh.launches, out[1] = out[2] = out[3] = out[4] = 0;
  if (!d->veh.ready()) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  unsigned long long cnt[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(cnt, d->veh.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost));
  for (int c = 0; c < 4; ++c) out[1 + c] = (int64_t)cnt[c];
  return HDSM_OK;
}

int hdsm_dswarm_track_stats(void* dswarm, int64_t out[3]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->track.q, out[1] = d->track.model_launches, out[2] = d->track.external_launches;
  return HDSM_OK;
}

}  // extern "C"
