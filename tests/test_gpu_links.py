"""Link faults in the device loop on the MI355X (hdsm_dswarm_set_links / _link_stats / _download_seen, k_deliver; include/hdsm_swarm.h):

  * deliveries: after every round k_deliver's seen / seen_has / seen_round / shift and the counters equal hdsm_link_deliver_host fed
    the downloaded truth records, bit for bit, on the crafted tables of tests/link_cases.py at H = 10 and 15;
  * identity: with an all-zero table the flight is the links-off flight bit for bit and seen is the plans buffer;
  * the twin flight: 8 agents, circle exchange, free space, 14 rounds, everyone 1 round late, agent 2 dark for rounds 3..8, agent 5
    out of order — against a HOST-DRIVEN twin: one SwarmShard of one agent per agent (first_id = a), each fed the view materialised
    in numpy for it (tests/link_cases.py PyLinkView + tests/shift_cases.py materialise) with its own slot fresh. Truth plans within
    1e-7 every round, statuses equal; time_aware on and off;
  * two local ranks on one device: the seen buffers of both ranks are the same bytes every round, the flight is the one-rank one;
  * the audit judges the truth records, not the seen ones.

Tolerances: those of tests/test_gpu_configs.py (device loop against host mirror): statuses equal, plans 1e-7."""
import numpy as np
import pytest

import link_cases as lc
import shift_cases as shc
from flight_harness import circle_flight, hdsm, raw  # noqa: F401  (hdsm: the module's fixture)
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

pytestmark = pytest.mark.gpu

N_ROB, RADIUS, PLAN_TOL = 8, 4.0, 1e-7


def scenario():
    return sc.circle_scenario(N_ROB, radius=RADIUS)


class _SeenView:
    def __init__(self, dsw):
        self.seen, self.seen_has, self.seen_round, self.shift = dsw.download_seen()


@pytest.mark.parametrize("n_hor,name", [(10, "out-of-order"), (10, "dark-longer-than-ring"), (10, "all-lost"), (10, "one-round-table"), (10, "delay-7"),
                                        (15, "out-of-order"), (15, "delay-7")])
@pytest.mark.parametrize("time_aware", [True, False], ids=["time-aware", "as-is"])
def test_deliveries_equal_the_host_function_bit_for_bit(hdsm, n_hor, name, time_aware):  # noqa: F811
    from multi_agent_pkgs_amd import lib
    prm = agile_params(n_hor, max_rows_static=18)
    fate = lc.crafted_tables(N_ROB)[name]
    sol, loop, dsw = circle_flight(hdsm, prm, *scenario())
    dsw.round()                                            # one round without links: the view of the call holds real plans
    plans0, has0 = raw(dsw), dsw.download(states=False)[1]
    dsw.set_links(fate, time_aware)
    step_plan = swarm.default_swarm_config().step_plan
    host = lib.LinkView(fate, N_ROB, n_hor, step_plan, time_aware, plans0, has0)
    s = _SeenView(dsw)
    assert s.seen.tobytes() == plans0.tobytes() and (s.seen_round == -1).all() and (s.shift == 0).all() and (s.seen_has == has0).all()
    rounds = fate.shape[0] + 9
    for r in range(rounds):
        dsw.round()
        host.deliver(raw(dsw))
        s = _SeenView(dsw)
        for got, want, what in ((s.seen, host.seen, "seen"), (s.seen_has, host.seen_has, "seen_has"), (s.seen_round, host.seen_round, "seen_round"),
                                (s.shift, host.shift, "shift")):
            assert got.tobytes() == want.tobytes(), (r, what)
    st = dsw.link_stats()
    c = host.counters
    assert st == dict(rounds=rounds, delivered=int(c[:, 0].sum()), lost=int(c[:, 1].sum()), max_age=int(c[:, 2].max())), (st, c.tolist())
    if name == "all-lost":
        assert st["delivered"] == 0 and st["lost"] == rounds * N_ROB and st["max_age"] == rounds
    dsw.set_links(None)                                    # off: the next round reads the plans buffer again, the view stays readable
    dsw.round()
    assert _SeenView(dsw).seen.tobytes() == s.seen.tobytes()
    dsw.close(), sol.close()


def test_an_all_zero_table_is_the_links_off_flight(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sol0, loop0, off = circle_flight(hdsm, prm, *scenario())
    sol1, loop1, on = circle_flight(hdsm, prm, *scenario())
    assert off.link_stats() == dict(rounds=0, delivered=0, lost=0, max_age=0)
    with pytest.raises(hdsm.HdsmError):
        off.download_seen()                                # nothing was allocated
    on.set_links(np.zeros((3, N_ROB), np.int8), True)
    for r in range(10):
        off.round(), on.round()
        assert raw(on).tobytes() == raw(off).tobytes(), r
        s = _SeenView(on)
        assert s.seen.tobytes() == raw(on).tobytes() and (s.shift == 0).all() and (s.seen_round == r).all(), r
        assert (on.download(states=False)[2] == off.download(states=False)[2]).all()
    assert on.link_stats() == dict(rounds=10, delivered=10 * N_ROB, lost=0, max_age=0)
    for x in (off, on, sol0, sol1):
        x.close()


def _twin_table():
    fate = np.ones((14, N_ROB), np.int8)                   # everyone one round late
    fate[3:9, 2] = -1                                      # agent 2 dark for rounds 3..8
    fate[4, 5], fate[5, 5] = 3, 1                          # agent 5: the record of round 5 lands in round 6, that of round 4 in round 7
    return fate


def _twin_flight(hdsm, prm, fate, time_aware, rounds):  # noqa: F811
    """The host-driven twin: per agent one SwarmShard of one agent and, every round, the view materialised for it."""
    cfg = swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(N_ROB, radius=RADIUS)
    rcfg = agile_ref_config()
    N = prm.n_hor
    solver_prm = agile_params(N, max_rows_static=18, warm_start=False)     # (one handle serves every agent's instance 0)
    sol = hdsm.Solver(solver_prm, 1, N_ROB)
    shards = [swarm.SwarmShard(prm, cfg, N_ROB, a, starts[a:a + 1], goals[a:a + 1]) for a in range(N_ROB)]
    truth, truth_has = np.zeros((N_ROB, N + 1, 9)), np.zeros(N_ROB, np.uint8)
    view = lc.PyLinkView(fate, N_ROB, N, cfg.step_plan, time_aware, truth, truth_has)
    out = []
    for r in range(rounds):
        new, new_has, status = truth.copy(), truth_has.copy(), np.zeros(N_ROB, np.int32)
        for a, sh in enumerate(shards):
            plans, has = shc.view_of(a, view.seen, view.seen_has, view.shift, truth, truth_has)
            plans = np.where(np.isnan(plans), 0.0, plans)
            sh.prepare_corridor()
            path, n_path = sh.reference_inputs(3)
            ref_full, _, pv = sol.reference(rcfg, np.array([a], np.int32), path, n_path, plans, has)
            sh.set_reference(ref_full, pv)
            inp = sh.prepare(plans, has)
            o = sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)
            pl, hl = sh.commit(o)
            new[a], new_has[a], status[a] = pl[0], hl[0], o["status"][0]
        truth, truth_has = new, new_has
        raw = truth.copy()
        raw[truth_has == 0] = 0.0
        raw[truth_has == 0, 0, 0] = lc.NAN_FRONT
        view.deliver(raw)
        out.append(dict(plans=truth.copy(), has=truth_has.copy(), status=status, seen_round=view.seen_round.copy(), shift=view.shift.copy(),
                        seen=view.seen.copy(), seen_has=view.seen_has.copy()))
    sol.close()
    return out


@pytest.fixture(scope="module")
def flights(hdsm):  # noqa: F811
    """the three device flights (links off, time-aware, as-is) of 14 rounds; per round the downloaded truth, statuses and view"""
    prm = agile_params(10, max_rows_static=18)
    fate = _twin_table()
    got = {}
    for key, ta in (("off", None), ("aware", True), ("as-is", False)):
        sol, loop, dsw = circle_flight(hdsm, prm, *scenario())
        if ta is not None:
            dsw.set_links(fate, ta)
        rounds = []
        for r in range(14):
            dsw.round()
            plans, has, status, _ = dsw.download(states=False)
            rec = dict(plans=plans, has=has, status=status)
            if ta is not None:
                s = _SeenView(dsw)
                rec.update(seen=s.seen, seen_has=s.seen_has, seen_round=s.seen_round, shift=s.shift)
            rounds.append(rec)
        got[key] = rounds
        dsw.close(), sol.close()
    return prm, fate, got


@pytest.mark.parametrize("key", ["aware", "as-is"])
def test_the_flight_is_the_host_driven_twin(hdsm, flights, key):  # noqa: F811
    prm, fate, got = flights
    twin = _twin_flight(hdsm, prm, fate, key == "aware", 14)
    worst = 0.0
    for r, (d, t) in enumerate(zip(got[key], twin)):
        assert (d["has"] == t["has"]).all() and (d["status"] == t["status"]).all(), (r, d["status"].tolist(), t["status"].tolist())
        assert (d["seen_round"] == t["seen_round"]).all() and (d["shift"] == t["shift"]).all() and (d["seen_has"] == t["seen_has"]).all(), r
        err = float(np.abs(d["plans"] - t["plans"]).max())
        worst = max(worst, err)
        assert err < PLAN_TOL, (r, err)
        assert np.nanmax(np.abs(np.where(np.isnan(d["seen"]), 0.0, d["seen"]) - np.where(np.isnan(t["seen"]), 0.0, t["seen"]))) < PLAN_TOL, r
    # what the table does to the view: agent 2's record ages through its outage, agent 5's late record of round 4 never shows
    ages = [int(r_ - d["seen_round"][2]) for r_, d in enumerate(got[key])]
    assert max(ages) == 7 and [int(d["seen_round"][5]) for d in got[key]][4:9] == [3, 3, 5, 6, 7]
    if key == "aware":
        assert max(int(d["shift"].max()) for d in got[key]) == min(7 * swarm.default_swarm_config().step_plan, prm.n_hor)
    else:
        assert all((d["shift"] == 0).all() for d in got[key])
    print(f"{key}: 14 rounds, max |plans - twin| {worst:.3e}")


def test_the_three_flights_differ(flights):
    _, _, got = flights
    dist = lambda a, b: max(float(np.abs(x["plans"] - y["plans"]).max()) for x, y in zip(got[a], got[b]))  # noqa: E731
    d_off, d_mode = dist("aware", "off"), dist("aware", "as-is")
    print(f"largest distance between flights: links on / off {d_off:.3f} m, time-aware / as-is {d_mode:.3f} m")
    assert d_off > 1e-3 and dist("as-is", "off") > 1e-3 and d_mode > 1e-3


def test_two_local_ranks_see_the_same_bytes_and_fly_the_one_rank_flight(hdsm, flights):  # noqa: F811
    prm, fate, got = flights
    starts, goals = sc.circle_scenario(N_ROB, radius=RADIUS)
    ranks = swarm.LocalRanks(prm, swarm.default_swarm_config(), N_ROB, 2, starts=starts, goals=goals)
    for d in ranks.dswarms:
        d.set_links(fate, True)
    for r in range(14):
        ranks.round(None)
        views = [_SeenView(d) for d in ranks.dswarms]
        for name in ("seen", "seen_has", "seen_round", "shift"):
            assert getattr(views[0], name).tobytes() == getattr(views[1], name).tobytes(), (r, name)
        one = got["aware"][r]
        assert (views[0].seen_round == one["seen_round"]).all() and (views[0].shift == one["shift"]).all(), r
        status = []
        for d in ranks.dswarms:
            plans, has, st, _ = d.download(states=False)
            status.append(st)
            assert (has == one["has"]).all() and np.abs(plans - one["plans"]).max() < PLAN_TOL, r
        assert (np.concatenate(status) == one["status"]).all(), r
    assert ranks.dswarms[0].link_stats() == ranks.dswarms[1].link_stats()
    ranks.close()


def test_the_audit_judges_what_was_flown_not_what_was_believed(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sol, loop, dsw = circle_flight(hdsm, prm, *scenario(), audit=True)
    dsw.set_links(_twin_table(), True)
    differs = 0
    for r in range(10):
        dsw.round()
        plans, has, _, _ = dsw.download(states=False)
        want = hdsm.flight_audit_host(plans, has, step_plan=swarm.default_swarm_config().step_plan, first=0, n_local=N_ROB, drone_radius=prm.drone_radius,
                                      drone_z_offset=prm.drone_z_offset)
        assert dsw.last_audit_round().tobytes() == want.tobytes(), r
        s = _SeenView(dsw)
        seen = np.where(np.isnan(s.seen), 0.0, s.seen)
        believed = hdsm.flight_audit_host(seen, s.seen_has, step_plan=swarm.default_swarm_config().step_plan, first=0, n_local=N_ROB,
                                          drone_radius=prm.drone_radius, drone_z_offset=prm.drone_z_offset)
        differs += believed.tobytes() != want.tobytes()
    assert differs >= 5                                    # everyone is a round late: the seen records are not the flown ones
    dsw.close(), sol.close()
