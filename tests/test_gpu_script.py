"""Scripted agents in the device loop on the MI355X (hdsm_dswarm_set_script / _script_stats, k_script; include/hdsm_swarm.h):

  * batch equals host: hdsm_script_records_batch equals hdsm_script_records_host (and the numpy restatement) bit for bit on every
    case of tests/script_cases.py;
  * records in the loop: 8 agents on the circle of tests/test_gpu_links.py (radius 4 m), ids 6 and 7 scripted — 6 holds at HOVER (on agent 0's straight path),
    7 flies a three-knot track along a chord with a turn. After every round of 14 the scripted slots of the raw plans buffer equal the
    host form's records bit for bit, state_curr in the history is states[step_plan], the flags are 1; H = 10 and 15, both modes;
  * the twin flight: one SwarmShard of one agent per flown agent, n_rob = 8, each fed the previous round's records with slots 6 and 7
    taken from the numpy restatement: statuses equal, plans within 1e-7, every round. Asserted from the twin alone: some flown agent's
    plan leaves the plan of the same twin flown with slots 6 and 7 absent by more than 0.05 m, and at most a quarter of the
    (agent, round) instances are HDSM_NO_SOLUTION;
  * sight against blindness: the same flight with every broadcast of ids 6 and 7 lost (set_links) flies into agent 6 — sigma_min
    against it below 0.5 — the sighted flight keeps strictly more, and every plan it solved satisfies the planes of hdsm_tasc_planes
    (a second handle) against the scripted records it was solved against within 1e-7;
  * dropout: five rounds unscripted (bit for bit the unscripted flight), then ids 6 and 7 hold where they are;
  * composition: two local ranks with one scripted tail id each; groups [0,4) [4,8) with id 7 scripted;
  * resources: k_script has no scratch and no LDS.

Tolerances: those of tests/test_gpu_links.py (device loop against host-driven twin): statuses equal, plans 1e-7."""
import numpy as np
import pytest

import script_cases as scs
from flight_harness import circle_flight, hdsm, raw  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import assert_no_scratch_no_lds
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

pytestmark = pytest.mark.gpu

N_ROB, N_FLY, RADIUS, PLAN_TOL, ROUNDS = 8, 6, 4.0, 1e-7, 14
# Agent 6 hovers on agent 0's straight path, 2 m in front of its start. (At the centre of the circle the flown agents give way to each
# other and a flight that does not see agent 6 still passes it at sigma 0.72 — measured on the CPU with the oracle as the solver, as
# were the twin's two conditions for this point: 0.84 m / 1.01 m from the twin without movers, no instance without a solution.)
HOVER = (20.0, 15.0, 1.5)
CHORD = np.array([[0.0, 20.8, 12.2, 1.5], [0.7, 19.0, 13.6, 1.5], [1.6, 16.4, 13.2, 1.5]])   # from agent 7's start, a turn, on


def script_tracks():
    return sc.stack_tracks(sc.hold_track(HOVER), CHORD)


def scenario():
    return sc.circle_scenario(N_ROB, radius=RADIUS)


def twin_flight(prm, solve, reference, tracks, predict, rounds, absent=False):
    """The host-driven twin: per FLOWN agent one SwarmShard of one agent; every round each is fed the records of the round before,
    slots 6 and 7 from the numpy restatement (absent: never there). solve(inp, plans, has) -> out; reference(ids, path, n_path,
    plans, has) -> (ref_full, path_vel) or None for the host mirror's own."""
    cfg = swarm.default_swarm_config()
    starts, goals = scenario()
    N = prm.n_hor
    shards = [swarm.SwarmShard(prm, cfg, N_ROB, a, starts[a:a + 1], goals[a:a + 1]) for a in range(N_FLY)]
    truth, truth_has = np.zeros((N_ROB, N + 1, 9)), np.zeros(N_ROB, np.uint8)
    out = []
    for r in range(rounds):
        new, new_has, status = truth.copy(), truth_has.copy(), np.zeros(N_ROB, np.int32)
        for a, sh in enumerate(shards):
            if reference is not None:
                sh.prepare_corridor()
                path, n_path = sh.reference_inputs(3)
                ref_full, pv = reference(np.array([a], np.int32), path, n_path, truth, truth_has)
                sh.set_reference(ref_full, pv)
            inp = sh.prepare(truth, truth_has)
            o = solve(inp, truth, truth_has)
            pl, hl = sh.commit(o)
            new[a], new_has[a], status[a] = pl[0], hl[0], o["status"][0]
        if not absent:
            new[N_FLY:], new_has[N_FLY:] = scs.records(tracks, N, cfg.step_plan, prm.dt, predict, r), 1
        truth, truth_has = new, new_has
        out.append(dict(plans=truth.copy(), has=truth_has.copy(), status=status))
    return out


def twin_conditions(seen, blind):
    """(the largest distance of a flown agent's plan from the blind twin's over the rounds, instances without a solution)"""
    dist = max(float(np.abs(s["plans"][:N_FLY, :, :3] - b["plans"][:N_FLY, :, :3]).max()) for s, b in zip(seen, blind))
    return dist, sum(int((s["status"][:N_FLY] == 2).sum()) for s in seen)


def _host(hdsm, tracks, prm, predict, q):  # noqa: F811
    return hdsm.script_records(tracks, prm.n_hor, swarm.default_swarm_config().step_plan, prm.dt, predict, q)


def test_the_batch_equals_the_host_form_bit_for_bit(hdsm):  # noqa: F811
    n = 0
    for name, knots, n_hor, step_plan, dt, predict, rnd in scs.cases():
        got = hdsm.script_records(knots, n_hor, step_plan, dt, predict, rnd, device=0)
        assert got.tobytes() == hdsm.script_records(knots, n_hor, step_plan, dt, predict, rnd).tobytes(), (name, n_hor, step_plan, predict, rnd)
        assert got.tobytes() == scs.expected(name, knots, n_hor, step_plan, dt, predict, rnd).tobytes(), (name, n_hor, step_plan, predict, rnd)
        n += 1
    assert n == 12 * 72
    L = hdsm.load()
    out = np.full((1, 11, 9), -7.0)
    bad = np.array([[[0.0, 0, 0, 0], [0.0, 1, 1, 1]]])
    assert L.hdsm_script_records_batch(0, 1, 2, bad, 10, 1, 0.1, 0, 0, out) == hdsm.HDSM_ERR_BAD_ARG and (out == -7.0).all()


@pytest.mark.parametrize("predict", [0, 1], ids=["truth", "constant-velocity"])
@pytest.mark.parametrize("n_hor", [10, 15])
def test_the_scripted_slots_are_the_host_records_every_round(hdsm, n_hor, predict):  # noqa: F811
    prm = agile_params(n_hor, max_rows_static=18)
    step_plan = swarm.default_swarm_config().step_plan
    tracks = script_tracks()
    sol, loop, dsw = circle_flight(hdsm, prm, *scenario())
    dsw.set_history(ROUNDS)
    assert dsw.script_stats() == dict(rounds=0, n_script=0, launches=0)
    dsw.set_script(tracks, predict)
    for r in range(ROUNDS):
        dsw.round()
        want = _host(hdsm, tracks, prm, predict, r)
        assert raw(dsw)[N_FLY:].tobytes() == want.tobytes(), r
        plans, has, status, _ = dsw.download(states=False)
        assert (has[N_FLY:] == 1).all() and (status[N_FLY:] == 0).all() and plans[N_FLY:].tobytes() == want.tobytes(), r
    hist, dropped = dsw.history(mirror=False)
    assert hist.shape == (ROUNDS, N_ROB, 9) and dropped == 0
    for r in range(ROUNDS):
        assert hist[r, N_FLY:].tobytes() == np.ascontiguousarray(_host(hdsm, tracks, prm, predict, r)[:, step_plan]).tobytes(), r
    assert dsw.script_stats() == dict(rounds=ROUNDS, n_script=2, launches=ROUNDS)
    assert (hist[-1, 6, :3] == HOVER).all() and np.abs(hist[-1, 7, :3] - CHORD[2, 1:]).max() < 1.0
    dsw.close(), sol.close()


def _sigma_against(hdsm, prm, plans, has, partner):  # noqa: F811
    """the smallest separation ratio of a flown agent against `partner` in one round of records"""
    best = np.inf
    for a in range(N_FLY):
        if has[a] and has[partner]:
            rec = hdsm.flight_audit_host(plans[[a, partner]], has[[a, partner]], step_plan=swarm.default_swarm_config().step_plan, first=0, n_local=1,
                                         drone_radius=prm.drone_radius, drone_z_offset=prm.drone_z_offset)
            best = min(best, float(np.sqrt(rec["sep2"][0])))
    return best


@pytest.fixture(scope="module")
def flights(hdsm):  # noqa: F811
    """The flight of 14 rounds at H = 10 with the audit and the history on: predict 0 and 1 as they are, and predict 0 with every
    broadcast of ids 6 and 7 lost. Per round the downloaded records, flags, statuses and the audit's round."""
    prm = agile_params(10, max_rows_static=18)
    tracks = script_tracks()
    got = {}
    for key, predict, blind in (("truth", 0, False), ("constant-velocity", 1, False), ("blind", 0, True)):
        sol, loop, dsw = circle_flight(hdsm, prm, *scenario(), audit=True)
        dsw.set_history(ROUNDS)
        dsw.set_script(tracks, predict)
        if blind:
            fate = np.zeros((1, N_ROB), np.int8)
            fate[0, N_FLY:] = -1
            dsw.set_links(fate, True)
        rounds = []
        for r in range(ROUNDS):
            dsw.round()
            plans, has, status, _ = dsw.download(states=False)
            rounds.append(dict(plans=plans, has=has, status=status, audit=dsw.last_audit_round()))
        got[key] = dict(rounds=rounds, hist=dsw.history(mirror=False)[0], report=dsw.flight_report(), predict=predict)
        dsw.close(), sol.close()
    return prm, tracks, got


@pytest.mark.parametrize("key", ["truth", "constant-velocity"])
def test_the_flight_is_the_host_driven_twin(hdsm, flights, key):  # noqa: F811
    prm, tracks, got = flights
    rcfg = agile_ref_config()
    sol = hdsm.Solver(agile_params(prm.n_hor, max_rows_static=18, warm_start=False), 1, N_ROB)   # (one handle serves every agent's instance 0)

    def solve(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def reference(ids, path, n_path, plans, has):
        full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has)
        return full, pv

    predict = got[key]["predict"]
    twin = twin_flight(prm, solve, reference, tracks, predict, ROUNDS)
    blind = twin_flight(prm, solve, reference, tracks, predict, ROUNDS, absent=True)
    sol.close()
    dist, unsolved = twin_conditions(twin, blind)
    print(f"{key}: the twin leaves the twin without movers by {dist:.3f} m, {unsolved} of {N_FLY * ROUNDS} instances without a solution")
    assert dist > 0.05 and 4 * unsolved <= N_FLY * ROUNDS
    worst = 0.0
    for r, (d, t) in enumerate(zip(got[key]["rounds"], twin)):
        assert (d["has"] == t["has"]).all() and (d["status"][:N_FLY] == t["status"][:N_FLY]).all(), (r, d["status"].tolist(), t["status"].tolist())
        err = float(np.abs(d["plans"] - t["plans"]).max())
        worst = max(worst, err)
        assert err < PLAN_TOL, (r, err)
    print(f"{key}: {ROUNDS} rounds, max |plans - twin| {worst:.3e}")


def test_sight_against_blindness(hdsm, flights):  # noqa: F811
    prm, tracks, got = flights
    step_plan = swarm.default_swarm_config().step_plan
    sigma = {key: min(_sigma_against(hdsm, prm, d["plans"], d["has"], 6) for d in got[key]["rounds"]) for key in ("truth", "blind")}
    overall = {key: swarm.flight_summary(got[key]["report"])["sigma_min"] for key in ("truth", "blind")}
    print(f"sigma_min against agent 6: sighted {sigma['truth']:.4f}, blind {sigma['blind']:.4f}; of the whole flight: {overall}")
    assert sigma["blind"] < 0.5                          # agent 6 stands on agent 0's straight path
    assert sigma["truth"] > sigma["blind"]
    # the sighted flight: every solved plan against the scripted records it was solved against
    sol2 = hdsm.Solver(prm, N_FLY, N_ROB)
    rounds, hist = got["truth"]["rounds"], got["truth"]["hist"]
    ids = np.arange(N_FLY, dtype=np.int32)
    checked, worst = 0, -np.inf
    for r in range(1, ROUNDS):
        before, now = rounds[r - 1], rounds[r]
        assert (before["has"][N_FLY:] == 1).all()
        planes = sol2.tasc_planes(ids, hist[r - 1, :N_FLY], before["plans"], before["has"])         # [6][N][8][4]
        for a in np.nonzero(now["status"][:N_FLY] != 2)[0]:
            for e in (0, 1):
                pts = now["plans"][a, e:prm.n_hor + e, :3]                                           # p_{i+e}
                viol = np.einsum("inc,ic->in", planes[a, :, N_FLY:, :3], pts) - planes[a, :, N_FLY:, 3]
                worst = max(worst, float(viol.max()))
                assert (viol < 1e-7).all(), (r, int(a), e, float(viol.max()))
            checked += 1
    sol2.close()
    print(f"{checked} solved plans against the movers' planes, largest n . p - b {worst:.3e}")
    assert checked >= N_FLY * ROUNDS - (N_FLY * ROUNDS) // 4 - N_FLY     # (at most a quarter without a solution; round 0 is not checked)
    # the audit has the movers as partners and as subjects
    assert any((d["audit"]["partner"][:N_FLY] >= N_FLY).any() for d in rounds) and all((d["audit"]["partner"][N_FLY:] >= 0).all() for d in rounds)
    assert (got["truth"]["report"]["rounds"] == ROUNDS).all() and step_plan >= 1


def test_an_agent_drops_out_in_flight(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sol0, loop0, plain = circle_flight(hdsm, prm, *scenario())
    sol1, loop1, dsw = circle_flight(hdsm, prm, *scenario())
    L = hdsm.load()
    assert L.hdsm_dswarm_set_script(dsw.h, 0, 1, None, 0) == 0 and dsw.script_stats() == dict(rounds=0, n_script=0, launches=0)   # a no-op
    for r in range(5):
        plain.round(), dsw.round()
        assert raw(dsw).tobytes() == raw(plain).tobytes(), r
    plans, has, status, _ = dsw.download(states=True)
    where = plans[N_FLY:, swarm.default_swarm_config().step_plan, :3].copy()
    assert (has == 1).all() and np.abs(loop1.shard.state()[0][N_FLY:] - where).max() == 0
    tracks = sc.stack_tracks(sc.hold_track(where[0]), sc.hold_track(where[1]))
    # every refusal leaves the flight untouched
    late = tracks.copy()
    late[0, 0, 0] = np.nan
    for bad, kw in ((np.concatenate([tracks] * 5)[:9], {}), (late, {}), (tracks, dict(predict=2)), (np.zeros((2, 257, 4)) + np.arange(257)[None, :, None], {})):
        with pytest.raises(hdsm.HdsmError) as e:
            dsw.set_script(bad, **kw)
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "hdsm_dswarm_set_script" in str(e.value)
    assert dsw.script_stats() == dict(rounds=0, n_script=0, launches=0)
    dsw.set_script(tracks)
    moved = 0.0
    for q in range(7):
        plain.round(), dsw.round()
        buf = raw(dsw)
        assert buf[N_FLY:].tobytes() == _host(hdsm, tracks, prm, 0, q).tobytes(), q
        assert (buf[N_FLY:, :, :3] == where[:, None, :]).all() and (buf[N_FLY:, :, 3:] == 0).all()
        moved = max(moved, float(np.abs(buf[:N_FLY] - raw(plain)[:N_FLY]).max()))
        assert dsw.script_stats() == dict(rounds=q + 1, n_script=2, launches=q + 1)
        if q == 3:                                         # shrinking is refused and leaves the flight untouched
            with pytest.raises(hdsm.HdsmError) as e:
                dsw.set_script(tracks[:1])
            assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
            assert L.hdsm_dswarm_set_script(dsw.h, 0, 1, None, 0) == hdsm.HDSM_ERR_BAD_ARG
    _, has, status, _ = dsw.download(states=False)
    assert (has == 1).all() and (status[N_FLY:] == 0).all()
    print(f"after the dropout the flown agents leave the unscripted flight by {moved:.3f} m")
    assert moved > 1e-3                                    # two agents that stopped are not two agents that fly on
    # new goals for everybody: the path step plans for the flown agents alone
    planned = dsw.path_stats()["planned"]
    dsw.set_goals(scenario()[1] + [0.5, 0.0, 0.0])
    dsw.round()
    assert dsw.path_stats()["planned"] - planned == N_FLY and raw(dsw)[N_FLY:].tobytes() == _host(hdsm, tracks, prm, 0, 7).tobytes()
    dsw.set_script(tracks)                                 # the same n_script: new tracks, tau starts again
    dsw.round()
    assert dsw.script_stats() == dict(rounds=1, n_script=2, launches=9) and raw(dsw)[N_FLY:].tobytes() == _host(hdsm, tracks, prm, 0, 0).tobytes()
    for x in (plain, dsw, sol0, sol1):
        x.close()
    # everybody scripted: the rank solves nothing and publishes eight tracks
    sol, loop, full = circle_flight(hdsm, prm, *scenario())
    starts, _ = scenario()
    every = sc.stack_tracks(*[sc.line_track(starts[k], HOVER, 1.0 + 0.25 * k) for k in range(N_ROB)])
    full.set_script(every, 1)
    for q in range(3):
        full.round()
        assert raw(full).tobytes() == _host(hdsm, every, prm, 1, q).tobytes(), q
    _, has, status, failed = full.download(states=False)
    assert (has == 1).all() and (status == 0).all() and failed == 0 and full.script_stats() == dict(rounds=3, n_script=8, launches=3)
    full.close(), sol.close()


def test_two_local_ranks_each_with_a_scripted_tail(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    starts, goals = scenario()
    ranks = swarm.LocalRanks(prm, swarm.default_swarm_config(), N_ROB, 2, starts=starts, goals=goals)
    tracks = [sc.line_track(starts[3], HOVER, 2.0)[None], CHORD[None]]            # id 3 (rank 0's tail) and id 7 (rank 1's)
    for d, t in zip(ranks.dswarms, tracks):
        d.set_script(t, 1)
    for r in range(8):
        ranks.round(None)
        (plans0, send0), (plans1, send1) = ranks.download_raw(0), ranks.download_raw(1)
        assert plans0.tobytes() == plans1.tobytes(), r
        assert plans0.tobytes() == np.concatenate([send0, send1]).tobytes(), r
        for rank, slot in ((0, 3), (1, 7)):
            assert plans0[slot].tobytes() == _host(hdsm, tracks[rank], prm, 1, r)[0].tobytes(), (r, slot)
        for d in ranks.dswarms:
            _, has, status, _ = d.download(states=False)
            assert (has == 1).all() and status[3] == 0
    assert [d.script_stats() for d in ranks.dswarms] == [dict(rounds=8, n_script=1, launches=8)] * 2
    ranks.close()


def test_a_mover_of_another_group_is_nobody(hdsm):  # noqa: F811
    """Groups [0,4) [4,8) on one rank, id 7 scripted through the middle of the circle: the agents of [0,4) fly bit for bit what they
    fly in a swarm of seven with groups [0,4) [4,7), and their audit never names 7."""
    prm = agile_params(10, max_rows_static=18)
    sol8, loop8, with7 = circle_flight(hdsm, prm, *scenario(), audit=True, groups=[0, 4, 8])
    sol7, loop7, without = circle_flight(hdsm, prm, *(x[:7] for x in scenario()), audit=True, groups=[0, 4, 7])
    with7.set_script(CHORD[None], 0)
    partners = set()
    for r in range(10):
        with7.round(), without.round()
        assert raw(with7)[:4].tobytes() == raw(without)[:4].tobytes(), r
        audit = with7.last_audit_round()
        partners |= set(audit["partner"][:4].tolist())
        assert audit["partner"][7] in (4, 5, 6), r          # ... while 7 itself is judged inside its own range
    assert partners <= {-1, 0, 1, 2, 3} and 7 not in partners
    rep = with7.group_report()
    assert rep["n_local"].tolist() == [4, 4] and rep["no_solution_last"][1] <= 3
    for x in (with7, without, sol8, sol7):
        x.close()


def test_k_script_uses_no_scratch_and_no_lds(tmp_path):
    assert_no_scratch_no_lds(tmp_path, "k_script")
