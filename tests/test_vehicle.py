"""A vehicle in the loop on the CPU (include/hdsm_swarm.h, csrc/vehicle_core.h): the host form against the plain-Python restatement of
tests/vehicle_cases.py bit for bit; the exact hover; the plant alone against closed forms; the defaults settle; every refusal; and the
host mirror flown with the oracle as the solver (8 agents on the 4 m circle, 14 rounds)."""
import ctypes as C
import math

import numpy as np
import pytest

import tracking_cases as tc
import vehicle_cases as vc
from multi_agent_pkgs_amd import lib, swarm
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import Vehicle, VehicleState, agile_params
from vehicle_cases import N_ROB, RECORDED, gusty, scenario

ROUNDS = 14
REST = np.array([1.0, -2.0, 1.5, 0, 0, 0, 0, 0, 0.0])


def test_the_host_form_against_the_restatement():
    n_cases, totals = 0, np.zeros(4, np.int64)
    for name, m, ids, q, step, dt, start, sps, planned, vss, names in vc.cases():
        got_vs, flown, dist, pose, stats = lib.vehicle_fly(m, ids, start, vc.command_array(sps), planned, vc.vstate_array(vss), step, dt, q)
        want_stats = np.zeros(4, np.int64)
        for k in range(len(ids)):
            w_vs, w_flown, w_d, _, w_pose, w_stats = vc.agent_round(m, ids[k], q, step, dt, start[k], sps[k], planned[k], vss[k])
            tag = (name, names[k])
            assert vc.same_vehicle(got_vs[k], w_vs), tag
            assert vc.bits(flown[k]) == vc.bits(w_flown) and vc.bits(dist[k]) == vc.bits(w_d), tag
            assert vc.same_pose(pose[k], w_pose), tag
            assert abs(((got_vs[k]["quat"] ** 2).sum()) - 1.0) <= 4 * np.spacing(1.0), tag
            want_stats += w_stats
            if names[k] == "not-finite-start":                                  # hold never looks at knot 0; along flies a NaN and re-seats
                assert w_stats[1] == (1 if m.feed == 1 else 0), tag
                if m.feed == 1:
                    assert vc.same_vehicle(got_vs[k], vc.seat(m, planned[k], 0.3)) and vc.bits(flown[k]) == vc.bits(planned[k]) and dist[k] == 0.0
            if names[k] == "clamps":
                assert w_stats[2] > 0 and w_stats[3] > 0, tag
        assert stats == tuple(int(x) for x in want_stats), name
        totals += want_stats
        n_cases += 1
    assert n_cases == vc.N_CASES
    assert totals[1] == vc.N_CASES // 2 and totals[2] > 0 and totals[3] > 0


def test_a_vehicle_that_is_not_finite_is_reseated_and_counted():
    m = vc.vehicle()
    vs = vc.seat(m, REST, 0.3)
    vs["vel"] = [0.0, math.inf, 0.0]
    sp = [[vc.setpoint(REST[:3], yaw=-0.4)]]
    got, flown, dist, pose, stats = lib.vehicle_fly(m, [5], [REST], vc.command_array(sp), [REST + 0.5], vc.vstate_array([vs]))
    assert stats == (0, 1, 0, 0) and dist[0] == 0.0 and vc.bits(flown[0]) == vc.bits(REST + 0.5)
    assert vc.same_vehicle(got[0], vc.seat(m, REST + 0.5, -0.4)) and pose[0]["valid"] == 1 and pose[0]["yaw"] == -0.4


def test_exact_hover():
    # the fixed point of the arithmetic as written: sqrt(fl(9.81 * 9.81)) is 9.81, 9.81 / 9.81 is 1, 1 - 2 (0 + 0) is 1
    assert math.sqrt(9.81 * 9.81) == 9.81 and 1.0 - 2.0 * (0.0 + 0.0) == 1.0 and 9.81 * 1.0 + -9.81 == 0.0
    for feed in (0, 1):
        m = vc.vehicle(feed=feed, acc_from=1)
        vs0 = lib.vehicle_seat(m, [REST], [0.0])
        assert vs0["quat"][0].tolist() == [0.0, 0.0, 0.0, 1.0] and vs0["thrust"][0] == 9.81 and not np.signbit(vs0["quat"][0]).any()
        sp = vc.command_array([[vc.setpoint(REST[:3])]])
        vs = vs0.copy()
        for r in range(100):
            vs, flown, dist, pose, stats = lib.vehicle_fly(m, [3], [REST], sp, [REST], vs, 1, 0.1, r)
            assert vs.tobytes() == vs0.tobytes() and vc.bits(flown[0]) == vc.bits(REST) and dist[0] == 0.0, (feed, r)
        assert stats == (1, 0, 0, 0)


def plant_only(**kw):
    zero = (0.0, 0.0, 0.0)
    return vc.vehicle(n_sub=100, kp=zero, kv=zero, k_att=zero, thrust_min=0.0, thrust_max=0.0, **kw)


def _fall(m, p0, v0, rounds=10):
    s = np.concatenate([p0, v0, [0.0, 0.0, vc.GZ]])
    vs = lib.vehicle_seat(m, [s], [0.4])                                        # (a - g = 0: thrust 0, which the clamps hold)
    assert vs["thrust"][0] == 0.0
    sp = vc.command_array([[vc.setpoint(p0)]])
    for r in range(rounds):
        vs, flown, _, _, _ = lib.vehicle_fly(m, [0], [s], sp, [s], vs, 1, 0.1, r)
        assert abs((vs["quat"][0] ** 2).sum() - 1.0) <= 4 * np.spacing(1.0)
    return flown[0]


def test_the_plant_alone_against_closed_forms():
    p0, v0 = np.array([1.0, 2.0, 30.0]), np.array([0.7, -0.3, 1.1])
    flown = _fall(plant_only(drag=(0.0, 0.0, 0.0)), p0, v0)                     # free fall, 1 s at h = 1 ms: RK4 is exact, rounding remains
    want = p0 + v0 * 1.0 + 0.5 * np.array([0.0, 0.0, vc.GZ]) * 1.0
    print("free fall |p - closed form|", np.abs(flown[:3] - want).max())
    assert np.abs(flown[:3] - want).max() <= 1e-12
    flown = _fall(plant_only(drag=(0.5, 0.5, 0.0)), p0, v0)                     # drag 0.5 / s: v_x(1 s) = v_0 exp(-0.5); (0.5 h)^5 / 120 per step
    rel = abs(flown[3] / (v0[0] * math.exp(-0.5)) - 1.0)
    print("drag |v_x / closed form - 1|", rel)
    assert rel <= 1e-12


def test_the_defaults_settle():
    """A 1 m step in x under hold with n_sub 10 and dt 0.1: under 1 % after 5 s, never beyond the step. A condition on the defaults."""
    m = lib.vehicle_default()
    assert (m.n_sub, m.feed, m.acc_from) == (10, 0, 0) and not any(m.wind) and not any(m.gust)
    vs = lib.vehicle_seat(m, [REST], [0.0])
    target = REST.copy()
    target[0] += 1.0
    sp = vc.command_array([[vc.setpoint(target[:3])]])
    worst = 0.0
    for r in range(50):
        vs, flown, _, _, _ = lib.vehicle_fly(m, [0], [REST], sp, [target], vs, 1, 0.1, r)
        worst = max(worst, float(np.abs(flown[:, :3] - target[:3]).max()))
    err = float(np.linalg.norm(flown[0, :3] - target[:3]))
    print(f"1 m step: error after 5 s {err:.3e} m, largest error on the way {worst:.4f} m")
    assert err < 0.01 and worst <= 1.0


def _bad_settings():
    def bad(**kw):
        m = vc.vehicle()
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, name)[v[0]] = v[1]
            else:
                setattr(m, name, v)
        return m

    return [bad(n_sub=0), bad(n_sub=1001), bad(feed=2), bad(feed=-1), bad(acc_from=2), bad(kp=(0, -1.0)), bad(kv=(1, -1e-9)), bad(k_att=(2, -1.0)),
            bad(tau_rate=0.0), bad(tau_thrust=-1.0), bad(thrust_min=-0.1), bad(thrust_min=5.0, thrust_max=4.0), bad(rate_max=(1, 0.0)),
            bad(drag=(0, -0.1)), bad(gust=(2, -1.0)), bad(wind=(0, math.nan)), bad(kp=(0, math.inf)), bad(tau_rate=math.nan),
            bad(thrust_max=math.inf), bad(rate_max=(2, math.inf))]


def test_every_argument_refusal_and_the_binding():
    L = lib.load()
    m = vc.vehicle()
    ids, st = np.arange(2, dtype=np.int32), np.ones((2, 9))
    sp, vs0 = vc.command_array([[vc.setpoint(REST[:3])]] * 2), lib.vehicle_seat(m, st, [0.0, 0.0])
    vs, flown = vs0.copy(), np.full((2, 9), -7.0)

    def rc(model=m, n=2, ids=ids, step=1, dt=0.1, q=0, start=st, sp=sp, end=st, vs=vs, flown=flown):
        return L.hdsm_vehicle_fly_host(model, n, ids, step, dt, q, start, sp, end, vs, flown, None, None, None)

    bads = [rc(model=b) for b in _bad_settings()] + [rc(model=None), rc(n=-1), rc(ids=None), rc(step=0), rc(step=10 ** 6), rc(dt=0.0), rc(dt=math.inf),
                                                      rc(q=-1), rc(q=2 ** 40 + 1), rc(start=None), rc(sp=None), rc(end=None), rc(vs=None), rc(flown=None)]
    assert all(r == lib.HDSM_ERR_BAD_ARG for r in bads), bads
    assert (flown == -7.0).all() and vs.tobytes() == vs0.tobytes()              # refused before anything is touched
    assert rc(n=0) == 0 and rc(q=2 ** 40) == 0 and not (flown == -7.0).any()
    assert L.hdsm_vehicle_seat_host(_bad_settings()[0], 2, st, np.zeros(2), vs) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_vehicle_seat_host(m, 2, None, np.zeros(2), vs) == lib.HDSM_ERR_BAD_ARG and L.hdsm_vehicle_default(None) == lib.HDSM_ERR_BAD_ARG
    assert [(n_, lib.VEHICLE_STATE.fields[n_][1]) for n_ in lib.VEHICLE_STATE.names] == [(n_, getattr(VehicleState, n_).offset) for n_, _ in VehicleState._fields_]
    assert [(n_, lib.VEHICLE.fields[n_][1]) for n_ in lib.VEHICLE.names] == [(n_, getattr(Vehicle, n_).offset) for n_, _ in Vehicle._fields_]
    assert C.sizeof(Vehicle) == 224 and C.sizeof(VehicleState) == 128


def _loop(oracle, prm):
    starts, goals = scenario()

    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    return swarm.SwarmLoop(prm, swarm.default_swarm_config(), N_ROB, solve=solve, starts=starts, goals=goals)


def test_the_mirror_refuses_what_cannot_be_flown(oracle):
    prm = agile_params(10, max_rows_static=18)
    shard = _loop(oracle, prm).shard
    m = gusty()

    def refused(fn, *a):
        with pytest.raises(lib.HdsmError) as e:
            fn(*a)
        return e.value.code == lib.HDSM_ERR_BAD_ARG

    assert refused(shard.vehicle_states)                                        # before the first setting
    assert refused(shard.set_vehicle, m)                                        # commands off
    shard.set_commands(True)
    shard.set_tracking(sc.gust_model(1, gust=(1.0, 1.0, 1.0)))
    assert refused(shard.set_vehicle, m)                                        # a tracking model on
    shard.set_tracking(None)
    for b in _bad_settings():
        assert refused(shard.set_vehicle, b)
    assert refused(shard.vehicle_states)                                        # ... and nothing was touched
    shard.set_vehicle(m)
    assert refused(shard.set_tracking, sc.gust_model(1))                        # the condition that could not occur before
    assert refused(shard.set_commands, False)
    ids = np.arange(N_ROB, dtype=np.int32)
    s0 = np.zeros((N_ROB, 9))
    s0[:, :3] = scenario()[0]
    assert shard.vehicle_states().tobytes() == lib.vehicle_seat(m, s0, np.zeros(N_ROB)).tobytes()
    given = s0 + 0.25                                                           # states from outside re-seat the masked vehicles
    mask = (ids % 2).astype(np.uint8)
    shard.set_states(given, mask)
    want = lib.vehicle_seat(m, np.where(mask[:, None] == 1, given, s0), np.zeros(N_ROB))
    assert shard.vehicle_states().tobytes() == want.tobytes()
    shard.set_vehicle(None)
    shard.set_tracking(sc.gust_model(1))                                        # off is off
    shard.set_tracking(None)
    shard.set_commands(False)


def test_the_mirror_flies_the_host_form(oracle):
    prm = agile_params(10, max_rows_static=18)
    m = gusty()
    step, dt = swarm.default_swarm_config().step_plan, prm.dt
    ids = np.arange(N_ROB, dtype=np.int32)
    mine, plain, unset = _loop(oracle, prm), _loop(oracle, prm), _loop(oracle, prm)
    mine.shard.set_commands(True), unset.shard.set_commands(True)
    mine.shard.set_vehicle(m)
    unset.shard.set_vehicle(m), unset.shard.set_vehicle(None), unset.shard.set_commands(False)
    vs = mine.shard.vehicle_states()
    state = np.zeros((N_ROB, 9))
    state[:, :3] = scenario()[0]
    recs = [tc.Record() for _ in range(N_ROB)]
    leaves, unsolved = 0.0, 0
    for r in range(ROUNDS):
        rec = []
        out = mine.step(record=rec)
        assert rec[0]["state"].tobytes() == state.tobytes(), r                  # x_0 is the vehicle's state of the round before
        plain.step(), unset.step()
        assert plain.plans_all.tobytes() == unset.plans_all.tobytes(), r        # set then unset is the mirror without it
        sp, pose, yaw = mine.shard.commands()
        has = mine.has_plan
        planned = np.where(has[:, None] == 1, mine.plans_all[:, step], state)
        vs, flown, dist, want_pose, _ = lib.vehicle_fly(m, ids, mine.plans_all[:, 0], sp, planned, vs, step, dt, r)
        assert mine.shard.vehicle_states().tobytes() == vs.tobytes(), r         # the state after the commit is the host form of the setpoints
        assert pose.tobytes() == want_pose.tobytes(), r
        assert (pose["quat"] == vs["quat"]).all() and (pose["yaw"] == yaw).all()
        for k in range(N_ROB):
            recs[k].book(float(dist[k]), tc.norm3(*(flown[k, 3:6] - planned[k, 3:6])))
        state = flown
        leaves = max(leaves, float(np.abs(mine.plans_all[:, :, :3] - plain.plans_all[:, :, :3]).max()))
        unsolved += int((out["status"] == 2).sum())
    assert tc.records_equal(mine.shard.track_records(), recs)
    assert not plain.shard.track_records()["rounds"].any()
    s = swarm.tracking_summary(mine.shard.track_records())
    print(f"leaves its vehicle-less copy by {leaves:.6f} m, {unsolved} of {N_ROB * ROUNDS} instances without a solution, tracking {s}")
    assert leaves > 1e-3                                                        # else the equality tests of the GPU suite are vacuous
    assert abs(leaves - RECORDED["leaves_by"]) < 5e-6 and unsolved == RECORDED["unsolved"]
    assert abs(s["mean"] - RECORDED["mean"]) < 5e-6 and abs(s["std"] - RECORDED["std"]) < 5e-6 and abs(s["max"] - RECORDED["max"]) < 5e-6
