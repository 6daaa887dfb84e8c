"""Missions in the device loop on the MI355X (hdsm_dswarm_set_mission / _mission_* / _fly, hdsm_mission_step_batch, k_mission,
k_mission_fold, the device-sized k_path / k_dmp; include/hdsm_swarm.h "missions"):

  * batch equals host: hdsm_mission_step_batch equals hdsm_mission_step_host byte for byte at n = 1, 63, 64, 65, 130 with every named
    case of tests/mission_cases.py in the last lane of a full wavefront and in a one-lane tail; the summary too;
  * the device loop against the host mirror that follows it, after every round of the shuttle, the square and the square in laps, in
    free space, in the forest (path period 0: only the mission makes anybody plan) and in clearance mode: records, summary, goal
    buffer, due agents, and behind the next round's path step every agent's path; the counters;
  * a scripted tail, a tracking model and a vehicle under the mission; groups; fly; the hand-over; off is off; resources."""
import numpy as np
import pytest

import corridor_oracle as co
import mission_cases as mc
from flight_harness import PLAN_TOL, MirroredRank, circle_flight, hdsm, model  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import assert_no_scratch_no_lds
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params

pytestmark = pytest.mark.gpu

PRM = agile_params(10, max_rows_static=18)


def test_the_batch_equals_the_host_form_byte_for_byte(hdsm):  # noqa: F811
    rng = np.random.default_rng(3)
    cases = mc.named_cases()
    for size in (1, 63, 64, 65, 130):
        for loop in (False, True):
            setting, rec, states, waypoints, count = mc.random_batch(rng, size, n_wp=int(rng.integers(1, 17)), loop=loop)
            goals, due = rng.uniform(-1, 1, (size, 3)), np.zeros(size, np.uint8)
            for rnd in (0, 1, 2):
                host = hdsm.mission_step(setting, rec, states, waypoints, count, round=rnd, goals=goals, due=due)
                dev = hdsm.mission_step(setting, rec, states, waypoints, count, round=rnd, goals=goals, due=due, device=0)
                mc.assert_same(dev, host, (size, loop, rnd))
                rec, goals, due = host[0], host[1], host[2]
    # every named case in lane 63 of a full wavefront (n = 64) and alone in the tail (n = 65, lane 0 of the second workgroup)
    for name, setting, rec1, s1, w1, c1, rnd in cases:
        for size in (64, 65):
            _, rec, states, waypoints, count = mc.random_batch(rng, size, n_wp=setting.n_wp, loop=bool(setting.loop), stall_rounds=3)
            rec[-1], states[-1], waypoints[-1], count[-1] = rec1[0], s1[0], w1[0], c1[0]
            host = hdsm.mission_step(setting, rec, states, waypoints, count, round=rnd)
            dev = hdsm.mission_step(setting, rec, states, waypoints, count, round=rnd, device=0)
            mc.assert_same(dev, host, (name, size))
            alone = hdsm.mission_step(setting, rec1, s1, w1, c1, round=rnd)
            assert dev[0][-1].tobytes() == alone[0][0].tobytes(), (name, size)
    L = hdsm.load()
    r, g, d = mc.blank_records(2), np.full((2, 3), 4.0), np.zeros(2, np.uint8)
    for over in (dict(n_wp=17), dict(n_wp=2, arrive_radius=0.0), dict(n_wp=2, dwell_rounds=0)):
        rc = L.hdsm_mission_step_batch(0, sc.mission_setting(**over), 2, 0, np.zeros((2, 9)), np.zeros((2, 17, 3)), np.ones(2, np.int32), r, g, d, None)
        assert rc == hdsm.HDSM_ERR_BAD_ARG and (g == 4.0).all() and r.tobytes() == mc.blank_records(2).tobytes()


# ---- the device loop with the host mirror that follows it ----
class MRank(MirroredRank):
    """tests/flight_harness.py's MirroredRank with a mission on both sides. Before a round the mirror has taken the device's flight —
    records, goals, due agents — and runs its own path step (prepare_corridor); behind the round the device's agents must hold the
    paths the mirror planned, and the mirror's commit must leave the records, the summary, the goals and the due agents of the device."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.setting, self.rounds_on, self.path_launches, self.planned, self.launches_that_planned = None, 0, 0, 0, 0

    def set_mission(self, setting, waypoints, count):
        self.dsw.set_mission(setting, waypoints, count), self.mirror.set_mission(setting, waypoints, count)
        self.setting = setting
        fly = self.n_fly
        assert self.dsw.mission_records()[:fly].tobytes() == self.mirror.mission_records()[:fly].tobytes() == mc.blank_records(fly).tobytes()
        due, goals = self.dsw.mission_due()
        assert due[:fly].all() and not due[fly:].any() and np.array_equal(goals[:fly], waypoints[:fly, 0])

    def before_round(self):
        super().before_round()
        if self.setting is None:
            return
        due, goals = self.mirror.mission_due()
        d_due, d_goals = self.dsw.mission_due()
        assert due.tobytes() == d_due.tobytes() and goals.tobytes() == d_goals.tobytes()     # (the hand-back brought flags and goals)
        self.due_before = due.copy()
        if self.n_fly:
            self.rounds_on, self.path_launches, self.planned = self.rounds_on + 1, self.path_launches + 1, self.planned + int(due[:self.n_fly].sum())
            self.launches_that_planned += int(due[:self.n_fly].any())
        self.mirror.prepare_corridor()                       # the mirror's own path step: whoever is due plans
        self.planned_agents = co.export_agents(self.mirror)[0]
        self.planned_rc = self.mirror.path_errors()[1]

    def feature_round(self, tag, ref_full, out, after, state):
        if self.setting is None:
            return
        fly, n = self.n_fly, self.n
        dev = co.export_agents(self.post)[0]                 # the device's agents behind the round
        dev_rc = self.post.path_errors()[1]
        for k in range(fly):                                 # behind this round's path step: the paths the mirror planned
            a, b = dev[k], self.planned_agents[k]
            assert a.n_path == b.n_path and bytes(a.path) == bytes(b.path) and dev_rc[k] == self.planned_rc[k], (tag, k, a.n_path, b.n_path)
        rec, m_rec = self.dsw.mission_records(), self.mirror.mission_records()
        assert rec[:fly].tobytes() == m_rec[:fly].tobytes(), (tag, rec[:fly], m_rec[:fly])
        assert rec[fly:].tobytes() == mc.blank_records(n - fly).tobytes(), tag          # a scripted agent flies no mission
        due, goals = self.dsw.mission_due()
        m_due, m_goals = self.mirror.mission_due()
        assert due[:fly].tobytes() == m_due[:fly].tobytes() and not due[fly:].any(), (tag, due, m_due)
        assert goals[:fly].tobytes() == m_goals[:fly].tobytes(), tag
        if fly == n:
            assert self.dsw.mission_summary() == self.mirror.mission_summary(), tag
        want = dict(launches=self.rounds_on, path_launches=self.path_launches, planned=self.planned)
        # (the agents flagged by THIS round are planned by the next one)
        assert self.dsw.mission_stats() == want, (tag, self.dsw.mission_stats(), want)


_WORLD = {}


def forest():
    """The small forest of flight_harness.forest_pair (seed 21, inflated), once per session: (world, origin)."""
    if not _WORLD:
        raw, origin = sc.forest_for_circle(4, seed=21)
        _WORLD["w"] = (sc.inflate(raw), origin)
    return _WORLD["w"]


def free_site(world, origin, points, clear=1):
    """An offset (dx, dy, 0) in half metres that puts every point of `points` [m][3] at least `clear` voxels away from every occupied
    voxel of its level — inside the forest (the pillars stand on whole metres), next to pillars, never in one."""
    occ = world >= 100
    for dx in np.arange(0.5, 16.0, 0.5):
        for dy in np.arange(0.5, 12.0, 0.5):
            v = np.floor((points + [dx, dy, 0.0] - origin) / sc.VOX).astype(int)
            if all(not occ[k, j - clear:j + clear + 1, i - clear:i + clear + 1].any() for i, j, k in v):
                near = any(occ[k, j - 8:j + 9, i - 8:i + 9].any() for i, j, k in v)
                if near:
                    return np.array([float(dx), float(dy), 0.0])
    raise AssertionError("no free site")


def mission_rank(hdsm, flight, where="free", n_script=0, extra=None):  # noqa: F811
    """(solver, rank, setting, starts, waypoints, count) of one of the flights of tests/mission_cases.py on one rank."""
    setting, starts, waypoints, count = flight
    setup = None
    if where != "free":
        world, origin = forest()
        shift = free_site(world, origin, np.concatenate([starts, waypoints.reshape(-1, 3)]))
        starts, waypoints = starts + shift, waypoints + shift

        def setup(shard, rank):
            shard.set_world(world, origin)
            if where == "dmp":
                shard.set_path_clearance(1.8)
            shard.set_path_period(0)
    if extra is not None:                                    # agents behind the mission's (a scripted tail)
        starts = np.concatenate([starts, extra])
        waypoints = np.concatenate([waypoints, np.repeat(extra[:, None, :], waypoints.shape[1], axis=1)])
        count = np.concatenate([count, np.ones(len(extra), np.int32)])
    goals = starts + [0.0, 0.5, 0.0]
    sol, loop, dsw = circle_flight(hdsm, PRM, starts, goals, setup=setup)
    rank = MRank(dsw, PRM, swarm.default_swarm_config(), starts, goals, n_fly=len(starts) - n_script)
    return sol, rank, setting, starts, waypoints, count


FLIGHTS = {"shuttle": (mc.shuttle, 60), "square": (mc.square, 45), "laps": (lambda: mc.square(loop=True), 70)}


@pytest.mark.parametrize("where", ["free", "forest"])
@pytest.mark.parametrize("name", list(FLIGHTS))
def test_the_device_loop_is_its_host_mirror(hdsm, name, where):  # noqa: F811
    make, rounds = FLIGHTS[name]
    sol, rank, setting, starts, waypoints, count = mission_rank(hdsm, make(), where)
    rank.set_mission(setting, waypoints, count)
    kinds = set()
    for r in range(rounds):
        rank.before_round()
        kinds.add(int(rank.due_before.sum()))
        rank.dsw.round()
        rank.after_round((name, where, r))
    rec, summary = rank.dsw.mission_records(), rank.dsw.mission_summary()
    assert {0, 4} <= kinds and (name != "shuttle" or kinds & {1, 2, 3}), kinds          # nobody due, some due, all due
    if name == "laps":
        assert summary["done"] == 0 and (rec["laps"] >= 1).all(), rec["laps"]
    elif where == "forest":                                  # (round the pillars a leg takes longer: the flight need not be over)
        assert (rec["arrivals"] >= 1).all() and summary["arrivals_total"] == rec["arrivals"].sum(), (summary, rec["arrivals"])
    else:
        assert summary["done"] == 4 and summary["makespan"] == rec["done_round"].max(), summary
    if where == "free":                                      # the arrivals the host mirror flies with the oracle (tests/test_mission.py)
        want = dict(shuttle=[[14, -1, -1, -1], [14, 28, -1, -1], [14, 28, 42, -1], [14, 28, 42, 56]], square=[[14, 28, 42]] * 4)
        if name in want:
            assert rec["arrive_round"][:, :len(want[name][0])].tolist() == want[name], rec["arrive_round"]
    stats = rank.dsw.path_stats()
    # the counters keep their meaning: agents planned, and the launches that planned somebody — not the empty device-sized ones
    assert stats["planned"] == rank.planned and stats["launches"] == rank.launches_that_planned < rank.path_launches, (stats, rank.path_launches)
    with pytest.raises(hdsm.HdsmError):
        rank.dsw.set_goals(starts)                           # refused while a mission is on


def test_the_square_in_clearance_mode_is_its_host_mirror(hdsm):  # noqa: F811
    sol, rank, setting, starts, waypoints, count = mission_rank(hdsm, mc.square(), "dmp")
    rank.set_mission(setting, waypoints, count)
    for r in range(45):
        rank.before_round()
        rank.dsw.round()
        rank.after_round(("dmp", r))
    assert rank.planned >= 12 and rank.dsw.mission_summary()["arrivals_total"] >= 8, (rank.planned, rank.dsw.mission_summary())


def test_a_scripted_agent_flies_no_mission(hdsm):  # noqa: F811
    sol, rank, setting, starts, waypoints, count = mission_rank(hdsm, mc.square(), n_script=1, extra=np.array([[20.0, 20.0, 1.5]]))
    rank.dsw.set_script(sc.hold_track((20.0, 20.0, 1.5)), 0)
    rank.set_mission(setting, waypoints, count)
    for r in range(20):
        rank.before_round()
        rank.dsw.round()
        rank.after_round(("script", r))
    rec = rank.dsw.mission_records()
    assert rec["arrivals"][:4].tolist() == [1, 1, 1, 1] and rec[4:].tobytes() == mc.blank_records(1).tobytes()
    assert rank.dsw.mission_summary()["flown"] == 4 and rank.planned == 8        # 4 at the start, 4 after the first arrival: never the tail
    assert rank.dsw.path_stats() == dict(planned=8, failed=0, launches=2)
    # the agents a mission flies are fixed when it is set: one more scripted agent is refused while it is on, new tracks are not
    two = sc.stack_tracks(sc.hold_track(starts[3]), sc.hold_track((20.0, 20.0, 1.5)))
    with pytest.raises(hdsm.HdsmError):
        rank.dsw.set_script(two, 0)
    rank.dsw.set_script(sc.hold_track((20.0, 20.0, 1.5)), 0)
    assert rank.dsw.mission_records().tobytes() == rec.tobytes() and rank.dsw.mission_summary()["flown"] == 4
    rank.dsw.set_mission(None)
    rank.dsw.set_script(two, 0)
    assert rank.dsw.script_stats()["n_script"] == 2


@pytest.mark.parametrize("what", ["tracking", "vehicle"])
def test_the_mission_judges_what_was_flown(hdsm, what):  # noqa: F811
    """With the tracking model of the harness, or a gusty vehicle, on both sides: the records equal the mirror's, which judged the
    FLOWN state_curr (the harness has compared it byte for byte), not the plan."""
    sol, rank, setting, starts, waypoints, count = mission_rank(hdsm, mc.shuttle())
    if what == "tracking":
        rank.dsw.set_tracking(model()), rank.mirror.set_tracking(model())
    else:
        m = sc.crazyflie_vehicle(seed=5, gust=(1.0, 1.0, 0.5))
        rank.set_commands(True)
        rank.dsw.set_vehicle(m), rank.mirror.set_vehicle(m)
    rank.set_mission(setting, waypoints, count)
    for r in range(30):
        rank.before_round()
        rank.dsw.round()
        rank.after_round((what, r))
    rec = rank.dsw.mission_records()
    plans = rank.dsw.download(states=False)[0]
    flown = np.array([list(a.state_curr) for a in co.export_agents(rank.mirror)[0]])
    assert np.abs(flown[:, :3] - plans[:4, 1, :3]).max() > 1e-4                   # (the flown state is not the planned one)
    judged = [k for k in range(4) if not rec["done"][k] and rec["last_arrival_round"][k] != 29]      # (still on the waypoint it was judged against)
    assert judged and all(abs(float(np.linalg.norm(flown[k, :3] - waypoints[k, rec["wp"][k]])) - rec["dist"][k]) < 1e-12 for k in judged), rec["dist"]


# ---- groups ----
def test_eight_shuttles_as_groups_and_a_crafted_partition(hdsm):  # noqa: F811
    setting, starts, waypoints, count = mc.shuttle()
    s8, g8, gs = sc.repeat_scenario(starts, starts + [0.0, 0.5, 0.0], 8)
    sol, loop, dsw = circle_flight(hdsm, PRM, s8, g8, groups=gs)
    dsw.set_mission(setting, np.tile(waypoints, (8, 1, 1)), np.tile(count, 8))
    rounds, last = dsw.fly(120, check_every=4)
    rec, groups = dsw.mission_records(), dsw.mission_groups()
    assert last["done"] == 32 and groups["makespan"].tolist() == [56] * 8 and rounds == 60, (rounds, last, groups["makespan"])
    _assert_fold(groups, rec, gs, 0, 32)
    # groups of 1, 63 and 66 agents on records crafted on the mirror and taken over: any done / stalled / laps pattern
    n, gs = 130, np.array([0, 1, 64, 130], np.int32)
    rng = np.random.default_rng(9)
    starts = np.stack([np.arange(n) * 3.0, np.zeros(n), np.full(n, 1.5)], axis=1)
    shard = swarm.SwarmShard(PRM, swarm.default_swarm_config(), n, 0, starts, starts + [0.0, 0.5, 0.0])
    shard.set_groups(gs)
    setting = sc.mission_setting(2, loop=False, dwell_rounds=1, stall_rounds=1, arrive_radius=0.3, arrive_speed=0.0)
    waypoints = np.repeat(starts[:, None, :], 2, axis=1)
    waypoints[:, 1, 1] += 1.0
    count = rng.integers(1, 3, n).astype(np.int32)
    shard.set_mission(setting, waypoints, count)
    N, P = PRM.n_hor, PRM.poly_hor
    for r in range(3):                                       # three commits: every agent stands on a waypoint of its own, or 1 m off it
        pos = waypoints[np.arange(n), rng.integers(0, 2, n)] + np.where(rng.random(n) < 0.3, 1.0, 0.0)[:, None] * [0.0, 0.0, 1.0]
        traj = np.zeros((n, N + 1, 9))
        traj[:, :, :3] = pos[:, None, :]
        shard.set_reference(np.concatenate([traj[:, :, :3], np.zeros((n, N + 1, 3))], axis=2), np.zeros(n))
        shard.commit(dict(traj=traj, ctrl=np.zeros((n, N, 3)), used=np.zeros((n, P), np.uint8), status=np.zeros(n, np.int32)))
    crafted = shard.mission_records()
    assert 0 < crafted["done"].sum() < n and crafted["stalled"].any() and len(set(crafted["arrivals"].tolist())) >= 3
    dsw = swarm.DeviceSwarm(shard, hdsm.Solver(PRM, n, n))
    assert dsw.mission_records().tobytes() == crafted.tobytes() and dsw.mission_summary() == shard.mission_summary()
    _assert_fold(dsw.mission_groups(), crafted, gs, 0, n)


def _assert_fold(groups, rec, gs, first, n_fly):
    """hdsm_dswarm_mission_groups against a numpy fold of the records."""
    for g in range(len(gs) - 1):
        lo, hi = max(gs[g], first), min(gs[g + 1], first + n_fly)
        r = rec[lo - first:hi - first]
        live = (r["stalled"] != 0) & (r["done"] == 0)
        want = (gs[g], gs[g + 1] - gs[g], len(r), int(r["done"].sum()), int(live.sum()), int(r["laps"].min()) if len(r) else 0,
                int(r["laps"].max()) if len(r) else 0, 0, int(r["arrivals"].sum()), int(r["done_round"].max()) if len(r) and r["done"].all() else -1)
        assert tuple(int(x) for x in groups[g]) == want, (g, groups[g], want)


# ---- fly ----
def _plain_flight(hdsm, flight, where="free"):  # noqa: F811
    sol, rank, setting, starts, waypoints, count = mission_rank(hdsm, flight, where)
    rank.dsw.set_mission(setting, waypoints, count)
    return sol, rank.dsw


def test_fly_stops_at_the_first_check_behind_the_end(hdsm):  # noqa: F811
    sol_a, a = _plain_flight(hdsm, mc.shuttle())
    rounds, last = a.fly(200, check_every=4)
    makespan = last["makespan"]
    assert last["done"] == last["flown"] == 4 and makespan == 56
    assert rounds == 4 * -(-(makespan + 1) // 4) == 60, (rounds, makespan)   # the first multiple of 4 not below makespan + 1
    sol_b, b = _plain_flight(hdsm, mc.shuttle())
    for _ in range(rounds):
        b.round()
    assert a.mission_records().tobytes() == b.mission_records().tobytes() and a.mission_summary() == b.mission_summary() == last
    pa, pb = a.download(states=False), b.download(states=False)
    assert (pa[1] == pb[1]).all() and np.abs(pa[0] - pb[0]).max() < PLAN_TOL
    assert a.mission_stats() == b.mission_stats()
    # max_rounds ends a flight that is not over
    sol_c, c = _plain_flight(hdsm, mc.shuttle())
    rounds, last = c.fly(10, check_every=4)
    assert rounds == 10 and last["done"] < last["flown"] and last["round"] == 9, (rounds, last)
    # refusals: no mission on; two ranks
    sol_d, loop_d, d = circle_flight(hdsm, PRM, *sc.circle_scenario(4, radius=4.0))
    with pytest.raises(hdsm.HdsmError):
        d.fly(10)
    d.set_mission(*mc.square()[:1], mc.square()[2], mc.square()[3])
    d.set_mission(None)
    with pytest.raises(hdsm.HdsmError):
        d.fly(10)
    setting, starts, waypoints, count = mc.square()
    s2 = np.concatenate([starts, starts + [0.0, 20.0, 0.0]])
    shard = swarm.SwarmShard(PRM, swarm.default_swarm_config(), 8, 0, s2[:4], s2[:4] + 0.5)
    two = swarm.DeviceSwarm(shard, hdsm.Solver(PRM, 4, 8), world_size=2)
    two.set_mission(setting, waypoints, count)
    with pytest.raises(hdsm.HdsmError) as e:
        two.fly(10)
    assert "world_size" in str(e.value) and two.mission_stats()["launches"] == 0


def test_fly_stops_on_a_stall(hdsm):  # noqa: F811
    """An agent whose only waypoint lies deep inside a solid block of the forest's world: its path step finds no free voxel, it keeps
    its old path, makes no progress and stalls; fly(stop_on_stall) returns before max_rounds, and without stop_on_stall it does not."""
    world, origin = forest()
    world = world.copy()
    start = np.array([[10.0, 10.0, 1.5]]) + free_site(world, origin, np.array([[10.0, 10.0, 1.5]]))
    centre = start[0] + [5.0, 0.0, 0.0]
    i, j, k = np.floor((centre - origin) / sc.VOX).astype(int)
    world[k - 8:k + 9, j - 8:j + 9, i - 8:i + 9] = 100       # 5.1 m across: no free voxel within the 6 shells of the path step

    def setup(shard, rank):
        shard.set_world(world, origin)
        shard.set_path_period(0)

    setting = sc.mission_setting(1, stall_rounds=6, stall_eps=0.05, arrive_radius=mc.R, arrive_speed=mc.V, dwell_rounds=mc.DWELL)
    flown = []
    for stop in (True, False):
        sol, loop, dsw = circle_flight(hdsm, PRM, start, start + [0.0, 0.5, 0.0], setup=setup)
        dsw.set_mission(setting, centre[None, None, :])
        rounds, last = dsw.fly(40, check_every=4, stop_on_stall=stop)
        flown.append(rounds)
        assert last["stalled"] == 1 and last["done"] == 0 and dsw.path_stats()["failed"] == 1, (stop, rounds, last, dsw.path_stats())
        assert dsw.mission_records()[0]["stall_events"] >= 1
    assert flown[0] < 40 and flown[0] % 4 == 0 and flown[1] == 40, flown


# ---- the hand-over ----
def test_a_mission_handed_over_goes_on_uninterrupted(hdsm):  # noqa: F811
    sol_a, a = _plain_flight(hdsm, mc.square())
    for _ in range(45):
        a.round()
    sol_b, b = _plain_flight(hdsm, mc.square())
    for _ in range(20):
        b.round()
    shard = b.shard
    b.download(states=True)
    at20 = b.mission_records()
    assert shard.mission_records().tobytes() == at20.tobytes() and shard.mission_summary() == b.mission_summary()
    plans, has = b.download(states=False)[:2]
    b.close()
    c = swarm.DeviceSwarm(shard, sol_b)
    c.upload_plans(plans[:4], has[:4])
    assert c.mission_records().tobytes() == at20.tobytes() and c.mission_summary()["round"] == 19
    for _ in range(25):
        c.round()
    # the records an uninterrupted flight gives: every integer field exactly; the two distances within PLAN_TOL — the second dswarm
    # starts its solver cold, and two flights that plan the same agree within PLAN_TOL only (tests/flight_harness.py), so the
    # doubles derived from the flown positions cannot be asked to agree byte for byte
    ra, rc = a.mission_records(), c.mission_records()
    for field in ra.dtype.names:
        if field in ("dist", "best_dist"):
            assert np.abs(rc[field] - ra[field]).max() < PLAN_TOL, (field, rc[field], ra[field])
        else:
            assert rc[field].tolist() == ra[field].tolist(), (field, rc[field], ra[field])
    assert rc["done_round"].tolist() == [42] * 4 and c.mission_summary() == a.mission_summary()
    # a flag pending at the hand-over still plans its agent: taken over right behind set_mission, everybody is due
    setting, starts, waypoints, count = mc.square()
    shard = swarm.SwarmShard(PRM, swarm.default_swarm_config(), 4, 0, starts, starts + [0.0, 0.5, 0.0])
    shard.set_mission(setting, waypoints, count)
    d = swarm.DeviceSwarm(shard, hdsm.Solver(PRM, 4, 4))
    assert d.mission_due()[0].all() and d.mission_stats() == dict(launches=0, path_launches=0, planned=0)
    d.download(states=True)                                  # ... and back again before any round: still pending on the mirror
    assert shard.mission_due()[0].all()
    d.round()
    assert d.mission_stats() == dict(launches=1, path_launches=1, planned=4) and not d.mission_due()[0].any()
    assert d.path_stats()["planned"] == 4


def test_off_is_off(hdsm):  # noqa: F811
    """A flight that never calls a mission entry point: no k_mission, no device-sized path launch, and the path step's launches are
    those of the same flight before missions existed — one per set_goals that changed a goal, none else (path period 0)."""
    starts, goals = sc.circle_scenario(8, radius=4.0)
    sol, loop, dsw = circle_flight(hdsm, PRM, starts, goals)
    for r in range(6):
        if r == 3:
            dsw.set_goals(starts)
        dsw.round()
    assert dsw.mission_stats() == dict(launches=0, path_launches=0, planned=0)
    assert dsw.path_stats() == dict(planned=8, failed=0, launches=1)
    with pytest.raises(hdsm.HdsmError):
        dsw.mission_records()
    assert not dsw.mission_due()[0].any() and np.array_equal(dsw.mission_due()[1], starts)
    # switched on and off again: the goals stay, set_goals works again, a pending flag goes to the host's list and still plans
    setting, s4, waypoints, count = mc.square()
    sol2, loop2, d2 = circle_flight(hdsm, PRM, s4, s4 + [0.0, 0.5, 0.0])
    d2.set_mission(setting, waypoints, count)
    d2.set_mission(None)
    assert d2.mission_due()[0].all() and np.array_equal(d2.mission_due()[1], waypoints[:, 0])
    d2.round()
    assert d2.path_stats() == dict(planned=4, failed=0, launches=1) and d2.mission_stats() == dict(launches=0, path_launches=0, planned=0)
    d2.set_goals(s4)
    d2.round()
    assert d2.path_stats()["planned"] == 8


def test_k_mission_uses_no_scratch_and_no_lds(tmp_path):
    assert_no_scratch_no_lds(tmp_path, "9k_missionE")
    assert_no_scratch_no_lds(tmp_path, "14k_mission_foldE")     # (the fold needs no LDS either: butterflies over the wavefront)
