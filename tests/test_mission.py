"""Missions on the CPU (csrc/mission_core.h, include/hdsm_swarm.h "missions"): hdsm_mission_step_host against the plain-Python
restatement of tests/mission_cases.py byte for byte, the argument checks, and the host mirror flying the shuttle, the square, the
square in laps and a held agent with the oracle as the solver."""
import numpy as np
import pytest

import mission_cases as mc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params


def test_the_host_form_equals_the_restatement_on_the_named_cases():
    seen = set()
    for name, setting, rec, states, waypoints, count, rnd in mc.named_cases():
        goals, due = np.full((1, 3), -7.0), np.zeros(1, np.uint8)
        want = mc.step(setting, rec, states, waypoints, count, rnd, goals, due)
        got = lib.mission_step(setting, rec, states, waypoints, count, round=rnd, goals=goals, due=due)
        mc.assert_same(got, want, name)
        r = got[0][0]
        seen.add(("arrived", bool(r["last_arrival_round"] == rnd)))
        seen.add(("done", int(r["done"]))), seen.add(("stalled", int(r["stalled"]))), seen.add(("laps", int(r["laps"])))
        seen.add(("events", int(r["stall_events"]))), seen.add(("not finite", bool(r["dist"] == -1.0)))
    # what the cases are there for did happen
    assert {("arrived", True), ("arrived", False), ("done", 1), ("stalled", 1), ("laps", 1), ("events", 2), ("not finite", True)} <= seen, seen
    by_name = {c[0]: c for c in mc.named_cases()}
    for name, arrives in (("on the radius, second round inside: arrives", True), ("just outside the radius", False), ("inside but too fast", False),
                          ("inside, fast, no speed test", True), ("speed exactly on the threshold", True)):
        _, setting, rec, states, waypoints, count, rnd = by_name[name]
        got = lib.mission_step(setting, rec, states, waypoints, count, round=rnd)
        assert bool(got[0][0]["arrivals"] == 1) == arrives and bool(got[2][0]) == arrives, name
        if arrives:
            assert np.array_equal(got[1][0], waypoints[0, 1]), name
    _, setting, rec, states, waypoints, count, rnd = by_name["one round outside resets the dwell"]
    assert lib.mission_step(setting, rec, states, waypoints, count, round=rnd)[0][0]["dwell"] == 0
    _, setting, rec, states, waypoints, count, rnd = by_name["done: nothing moves"]
    assert lib.mission_step(setting, rec, states, waypoints, count, round=rnd)[0].tobytes() == rec.tobytes()


@pytest.mark.parametrize("loop", [False, True])
def test_the_host_form_equals_the_restatement_on_random_batches(loop):
    rng = np.random.default_rng(11 + loop)
    arrived = stalled = bad = 0
    for trial in range(6):
        setting, rec, states, waypoints, count = mc.random_batch(rng, 97, n_wp=int(rng.integers(1, 17)), loop=loop)
        goals, due = rng.uniform(-1, 1, (97, 3)), np.zeros(97, np.uint8)
        for rnd in range(3):   # (the same states three times: dwell and since move on)
            want = mc.step(setting, rec, states, waypoints, count, rnd, goals, due)
            got = lib.mission_step(setting, rec, states, waypoints, count, round=rnd, goals=goals, due=due)
            mc.assert_same(got, want, (trial, rnd))
            rec, goals, due = got[0], got[1], got[2]
            arrived += got[3]["arrivals"]
        stalled += int(rec["stalled"].sum())
        bad += int((rec["dist"] == -1.0).sum())
    assert arrived > 50 and stalled > 50 and bad > 5, (arrived, stalled, bad)


def test_the_makespan_is_minus_one_until_the_last_agent_is_done():
    setting = sc.mission_setting(1, dwell_rounds=1)
    waypoints = np.zeros((3, 1, 3))
    states = np.zeros((3, 9))
    states[:, 0] = [0.0, 5.0, 5.0]
    rec = mc.blank_records(len(states))
    rec, _, _, s = lib.mission_step(setting, rec, states, waypoints, round=0)
    assert (s["done"], s["makespan"], s["arrivals"]) == (1, -1, 1)
    states[1, 0] = 0.0
    rec, _, _, s = lib.mission_step(setting, rec, states, waypoints, round=1)
    assert (s["done"], s["makespan"], s["arrivals"], s["arrivals_total"]) == (2, -1, 1, 2)
    states[2, 0] = 0.0
    rec, _, _, s = lib.mission_step(setting, rec, states, waypoints, round=4)
    assert (s["done"], s["makespan"], s["flown"]) == (3, 4, 3) and rec["done_round"].tolist() == [0, 1, 4]
    assert lib.mission_step(setting, rec[:0], states[:0], waypoints[:0], round=0)[3]["makespan"] == -1   # (nobody: the identity)


def test_arguments_out_of_bounds_are_refused_with_nothing_changed():
    good = dict(n_wp=2, dwell_rounds=2, arrive_radius=0.3)
    waypoints, states = np.zeros((2, 2, 3)), np.zeros((2, 9))
    rec = mc.blank_records(len(states))
    L = lib.load()
    for over, count in ((dict(n_wp=0), [1, 1]), (dict(n_wp=17), [1, 1]), ({}, [1, 3]), ({}, [0, 1]), (dict(arrive_radius=0.0), [1, 1]),
                        (dict(arrive_radius=-1.0), [1, 1]), (dict(dwell_rounds=0), [1, 1]), (dict(arrive_radius=float("nan")), [1, 1])):
        setting = sc.mission_setting(**dict(good, **over))
        r, g, d = rec.copy(), np.full((2, 3), 4.0), np.zeros(2, np.uint8)
        summary = lib.MissionSummary()
        rc = L.hdsm_mission_step_host(setting, 2, 0, states, waypoints, np.asarray(count, np.int32), r, g, d, summary)
        assert rc == lib.HDSM_ERR_BAD_ARG, (over, count)
        assert r.tobytes() == rec.tobytes() and (g == 4.0).all() and not d.any() and summary.round == 0, (over, count)
    # the mirror refuses the same settings and stays without a mission
    shard = swarm.SwarmShard(agile_params(10, max_rows_static=18), swarm.default_swarm_config(), 2, 0, np.zeros((2, 3)), np.ones((2, 3)))
    for over, count in ((dict(n_wp=17), [1, 1]), ({}, [1, 3]), (dict(dwell_rounds=0), [1, 1])):
        rc = L.hdsm_swarm_set_mission(shard.h, sc.mission_setting(**dict(good, **over)), np.zeros((2, 17, 3)), np.asarray(count, np.int32))
        assert rc == lib.HDSM_ERR_BAD_ARG
    with pytest.raises(lib.HdsmError):
        shard.mission_records()
    assert not shard.mission_due()[0].any()


# ---- the host mirror flown with the oracle as the solver ----
def _oracle_loop(oracle, prm, starts, goals):
    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    return swarm.SwarmLoop(prm, swarm.default_swarm_config(), len(starts), solve=solve, starts=starts, goals=goals)


def _fly(oracle, setting, starts, waypoints, count, rounds, stop_when_done=True):
    """The mirror's flight: (loop, records, summary, rounds flown, minimum separation, the nearest a tested quantity came to its threshold)."""
    prm = agile_params(10, max_rows_static=18)
    loop = _oracle_loop(oracle, prm, starts, starts + [0.0, 0.5, 0.0])
    loop.shard.set_mission(setting, waypoints, count)
    due, goals = loop.shard.mission_due()
    assert due.all() and np.array_equal(goals, waypoints[:, 0])
    n, min_sep, margin, flown = len(starts), np.inf, np.inf, 0
    rec = mc.blank_records(n)
    assert loop.shard.mission_records().tobytes() == rec.tobytes()
    goals, due = goals.copy(), np.zeros(n, np.uint8)
    for r in range(rounds):
        out = loop.step()
        flown += 1
        assert (out["status"] != 2).all(), (r, out["status"])
        assert loop.shard.path_errors()[0] == 0 and loop.shard.corridor_errors()[0] == 0, r
        # the mirror's commit judged the states it left: the restatement on the published records' flown state gives the same bytes
        states = loop.plans_all[:, loop.shard.cfg.step_plan]
        rec, goals, _, want = mc.step(setting, rec, states, waypoints, count, r, goals, due)
        got, summary = loop.shard.mission_records(), loop.shard.mission_summary()
        assert got.tobytes() == rec.tobytes() and summary == want, (r, summary, want)
        assert np.array_equal(loop.shard.mission_due()[1], goals), r
        pos = states[:, :3]
        if n > 1:
            min_sep = min(min_sep, (np.linalg.norm(pos[:, None] - pos[None], axis=2) + np.eye(n) * 1e9).min())
        live = got["done"] == 0
        speed = np.linalg.norm(states[:, 3:6], axis=1)
        margin = min([margin] + [abs(got["dist"][k] - mc.R) for k in range(n) if live[k]] + [abs(speed[k] - mc.V) for k in range(n) if live[k]])
        if stop_when_done and summary["done"] == n:
            break
    return loop, got, summary, flown, min_sep, margin


def test_the_mirror_flies_the_shuttle_to_completion(oracle):
    setting, starts, waypoints, count = mc.shuttle()
    loop, rec, summary, flown, min_sep, margin = _fly(oracle, setting, starts, waypoints, count, 80)
    print("shuttle: arrivals", rec["arrive_round"][:, :4].tolist(), "rounds", flown, "min separation %.3f" % min_sep, "margin %.4f" % margin)
    assert summary["done"] == 4 and (rec["done"] == 1).all() and flown <= 80, (summary, flown)
    assert summary["makespan"] == rec["done_round"].max() == flown - 1
    assert np.array_equal(loop.shard.mission_due()[1], mc.last_waypoints(waypoints, count))
    assert rec["arrivals"].tolist() == [1, 2, 3, 4] and not rec["stalled"].any()


def test_the_mirror_flies_the_square_to_completion(oracle):
    setting, starts, waypoints, count = mc.square()
    loop, rec, summary, flown, min_sep, margin = _fly(oracle, setting, starts, waypoints, count, 60)
    print("square: arrivals", rec["arrive_round"][:, :3].tolist(), "rounds", flown, "min separation %.3f" % min_sep, "margin %.4f" % margin)
    assert summary["done"] == 4 and flown <= 60, (summary, flown)
    assert np.array_equal(loop.shard.mission_due()[1], mc.last_waypoints(waypoints, count))
    assert min_sep > 0.5


def test_the_mirror_flies_the_square_in_laps(oracle):
    setting, starts, waypoints, count = mc.square(loop=True)
    loop, rec, summary, flown, min_sep, margin = _fly(oracle, setting, starts, waypoints, count, 100, stop_when_done=False)
    print("laps: arrivals", rec["arrive_round"][:, :3].tolist(), "laps", rec["laps"].tolist(), "min separation %.3f" % min_sep)
    assert flown == 100 and rec["laps"].tolist() == [2, 2, 2, 2] and summary["done"] == 0 and summary["makespan"] == -1
    assert min_sep > 0.5


def test_a_held_agent_stalls_at_round_five_and_recovers(oracle):
    """One agent, a 3 m leg, stall_rounds 5, stall_eps 0.05: set_states puts it back on its start after every round for 8 rounds. Round
    0 is progress against best_dist (a reset record has seen no distance yet), rounds 1 .. 5 are not: stalled at mission round 5
    exactly. Released, the first round with progress clears it — stall_events is 1 there — and the agent arrives.
    Measured with the oracle: the first round with progress is mission round 10 (from rest the position of the first two states does
    not move), the closest pass is 0.0195 m at round 18 at 1.16 m/s, the agent then settles inside the radius for six rounds without
    coming closer — with stall_rounds = 5 that raises a second stall at round 23 — and arrives at round 25 with stall_events == 2."""
    prm = agile_params(10, max_rows_static=18)
    start = np.array([[10.0, 10.0, 1.5]])
    waypoints = start[:, None, :] + [3.0, 0.0, 0.0]
    setting = sc.mission_setting(1, stall_rounds=5, stall_eps=0.05, arrive_radius=mc.R, arrive_speed=mc.V, dwell_rounds=mc.DWELL)
    loop = _oracle_loop(oracle, prm, start, start + [0.0, 0.5, 0.0])
    loop.shard.set_mission(setting, waypoints)
    held = np.concatenate([start, np.zeros((1, 6))], axis=1)
    seen = []
    for r in range(8):
        loop.step()
        rec = loop.shard.mission_records()[0]
        seen.append((int(rec["stalled"]), int(rec["since"])))
        loop.shard.set_states(held)
    assert [s for s, _ in seen] == [0, 0, 0, 0, 0, 1, 1, 1], seen
    assert [q for _, q in seen] == [0, 1, 2, 3, 4, 5, 6, 7], seen
    assert loop.shard.mission_summary()["stalled"] == 1
    first_progress = None
    for r in range(8, 60):
        best = float(loop.shard.mission_records()[0]["best_dist"])
        loop.step()
        rec = loop.shard.mission_records()[0]
        if first_progress is None:
            if rec["dist"] < best - 0.05:     # the first round with progress: the stall is cleared, and it was the only one
                first_progress = r
                assert rec["stalled"] == 0 and rec["stall_events"] == 1 and rec["since"] == 0, (r, rec)
            else:
                assert rec["stalled"] == 1 and rec["stall_events"] == 1, (r, rec)
        if rec["done"]:
            break
    assert first_progress is not None and rec["done"] == 1 and rec["arrivals"] == 1, (first_progress, rec)
