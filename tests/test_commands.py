"""Commands for the vehicle on the CPU (include/hdsm_swarm.h, csrc/command_core.h — the source k_command runs): the library's own atan2
and sincos against numpy.longdouble on the fixed sample of tests/command_cases.py and the special cases against math.atan2;
hdsm_command_host against the restatement of that file on crafted agents that reach every branch; the level vehicle, whose matrix is
a rotation; every argument refusal; the binding; and the host mirror flown with the oracle as the solver (the 8-agent exchange, 30
rounds) against hdsm_swarm_yaw, which uses libm, on a twin flight.

Tolerances (command_cases.py): E = 4.33e-16 is the measured error of the own functions; the sample asserts 2 E, a comparison with
the libm restatement 4 E plus 8 ulp of the compared value, the yaw of a flight 2 E plus 8 ulp (yaw' = (1 - c) yaw + c yaw_ref with
c = k_p_yaw dt < 1: a difference never grows)."""
import ctypes as C
import math

import numpy as np
import pytest

import command_cases as cc
from multi_agent_pkgs_amd import lib, swarm
from multi_agent_pkgs_amd.params import K_P_YAW, YAW_IDX, Command, agile_params


def test_own_atan2_and_sincos_against_long_double():
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble is not the 80-bit format here"
    y, x = cc.atan2_sample()
    assert y.size == 257 * 257 - 1 + 20000 + 42 + 24
    err_atan2 = float(np.abs(lib.command_atan2(y, x).astype(LD) - np.arctan2(y.astype(LD), x.astype(LD))).max())
    v = cc.sincos_sample()
    assert v.size == 20000 + 3 * 12733 + 2 and np.abs(v).max() <= 1e4 + 1e-8
    s, c = lib.command_sincos(v)
    err_sin, err_cos = float(np.abs(s.astype(LD) - np.sin(v.astype(LD))).max()), float(np.abs(c.astype(LD) - np.cos(v.astype(LD))).max())
    print(f"max abs error: atan2 {err_atan2:.3e}, sin {err_sin:.3e}, cos {err_cos:.3e}; E = {cc.E:.3e}")
    assert max(err_atan2, err_sin, err_cos) <= 2 * cc.E and cc.E < 1e-12
    # the special cases, exactly C's: +-0, the axes, infinities; a NaN in gives a NaN
    for y0, x0 in cc.SPECIAL:
        got, want = float(lib.command_atan2([y0], [x0])[0]), math.atan2(y0, x0)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (y0, x0, got, want)
    for y0, x0 in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.nan, np.inf), (0.0, np.nan)):
        assert np.isnan(lib.command_atan2([y0], [x0])[0])
    # beyond the bound that is pinned: unchanged up to 2^20, NaN from there on and for what is not finite — never a wrong finite value
    far = np.random.default_rng(4).uniform(-2.0 ** 20, 2.0 ** 20, 2000)
    s, c = lib.command_sincos(far)
    assert float(max(np.abs(s.astype(LD) - np.sin(far.astype(LD))).max(), np.abs(c.astype(LD) - np.cos(far.astype(LD))).max())) <= 2 * cc.E
    s, c = lib.command_sincos([2.0 ** 20, -2.0 ** 20, 1e300, np.inf, -np.inf, np.nan])
    assert np.isnan(s).all() and np.isnan(c).all()


def _restated(case, step_plan, dt=0.1, yaw_idx=YAW_IDX, k_p=K_P_YAW):
    return [cc.agent_round(case["yaw"][k], case["n_ref"][k], case["ref_point"][k], case["state_before"][k], case["records"][k], int(case["valid"][k]),
                           case["state_after"][k], step_plan, dt, yaw_idx, k_p) for k in range(len(case["yaw"]))]


@pytest.mark.parametrize("step_plan", [1, 3])
def test_the_host_form_against_the_restatement(step_plan):
    case, names = cc.crafted()
    yaw, sp, pose, stats = lib.command(**case, step_plan=step_plan)
    want = _restated(case, step_plan)
    branches = set()
    for k, (name, (w_yaw, w_stepped, w_sp, w_pose)) in enumerate(zip(names, want)):
        assert abs(yaw[k] - w_yaw) <= cc.tol(w_yaw), (name, yaw[k], w_yaw)
        assert w_stepped or yaw[k] == case["yaw"][k], name                                  # the branch of the yaw step (and the counters below)
        for j in range(step_plan):
            assert cc.close(sp[k, j], w_sp[j]), (name, j, sp[k, j], w_sp[j])
        assert cc.close(pose[k], w_pose), (name, pose[k], w_pose)
        assert pose[k]["pad"] == 0 and pose[k]["reserved0"] == 0.0
        branches.add(w_pose["branch"])
    assert branches >= {"T", 0, 1, 2}, branches                                              # Eigen's rule: every branch was reached
    assert stats == (sum(w[1] for w in want), sum(not w[1] for w in want)) and stats[0] > 5 and stats[1] > 5
    at = {n: k for k, n in enumerate(names)}
    # the 0.1 rule is strict; a missing reference point, a state that is not finite: the yaw stays bit for bit
    assert yaw[at["below-0.1"]] == yaw[at["at-0.1"]] == 0.7 and yaw[at["above-0.1"]] != 0.7
    for name in ("n_ref-equals-yaw_idx", "n_ref-zero", "before-nan", "before-inf"):
        assert yaw[at[name]] == case["yaw"][at[name]], name
    # the wrap: from 3.0 towards -3.0 the yaw goes UP through pi, not back through 0
    assert yaw[at["wrap-down"]] > 3.0 and yaw[at["wrap-up"]] < -3.0
    # a state or a knot that is not finite: valid 0 and every other field zero
    zero = np.zeros(1, lib.COMMAND)[0]
    for name in ("after-inf", "after-nan-acc"):
        assert pose[at[name]].tobytes() == zero.tobytes() and sp[at[name], 0]["valid"] == 1, name
    k = at["knot-nan"]
    assert sp[k, 0]["valid"] == 1 and pose[k]["valid"] == 1                                  # (knot 2 holds the NaN)
    assert step_plan == 1 or (sp[k, 1].tobytes() == zero.tobytes() and sp[k, 2]["valid"] == 1)
    # no plan yet: the position held, velocity and acceleration zero, a hover attitude; the fallback is marked
    k = at["no-plan"]
    for cmd in [pose[k]] + [sp[k, j] for j in range(step_plan)]:
        assert cmd["valid"] == 0 and (cmd["pos"] == case["state_after"][k, :3]).all() and not cmd["vel"].any() and not cmd["acc"].any()
        assert abs(np.linalg.norm(cmd["quat"]) - 1.0) < 1e-15
    assert pose[at["fallback"]]["valid"] == 2 and (sp[at["fallback"], :]["valid"] == 2).all()
    # the setpoints are knots 1 .. step_plan of the record, bit for bit, and carry the yaw AFTER the step
    k = at["behind"]
    for j in range(step_plan):
        assert np.concatenate([sp[k, j]["pos"], sp[k, j]["vel"], sp[k, j]["acc"]]).tobytes() == case["records"][k, j + 1].tobytes()
        assert sp[k, j]["yaw"] == yaw[k] != 0.0


def test_a_level_vehicle_gets_a_rotation():
    """a_x = a_y = 0 and a_z > -9.81: z_b = e_z, the matrix is the rotation by yaw about z — a unit quaternion that takes e_x onto
    (cos yaw, sin yaw, 0)."""
    rng = np.random.default_rng(8)
    n = 200
    yaws = np.concatenate([rng.uniform(-1e4, 1e4, n - 8), [0.0, math.pi, -math.pi, math.pi / 2, 3.0, -3.0, 2.0 * math.pi / 3, 1e4]])
    rec = np.zeros((n, 11, 9))
    rec[:, :, 8] = rng.uniform(-9.8, 15.0, n)[:, None]
    case = dict(yaw=yaws, n_ref=np.zeros(n, np.int32), ref_point=np.zeros((n, 3)), state_before=np.zeros((n, 9)), records=rec, valid=np.ones(n, np.int32),
                state_after=rec[:, 1].copy())
    yaw, sp, pose, stats = lib.command(**case)
    assert stats == (0, n) and (yaw == yaws).all() and (pose["valid"] == 1).all()
    for q, y in zip(pose["quat"], yaws):
        x_, y_, z_, w_ = (float(v) for v in q)
        assert abs(math.sqrt(x_ * x_ + y_ * y_ + z_ * z_ + w_ * w_) - 1.0) <= 4 * np.spacing(1.0)
        ex = (1.0 - 2.0 * (y_ * y_ + z_ * z_), 2.0 * (x_ * y_ + w_ * z_), 2.0 * (x_ * z_ - w_ * y_))      # the first column of R(q)
        assert max(abs(ex[0] - math.cos(y)), abs(ex[1] - math.sin(y)), abs(ex[2])) <= 4 * cc.E, (y, ex)


def test_every_argument_refusal_and_the_binding():
    L = lib.load()
    case, _ = cc.crafted()
    n = len(case["yaw"])
    pose = np.zeros(n, lib.COMMAND)
    keep = case["yaw"].copy()

    def rc(n=n, n_hor=10, step=1, dt=0.1, idx=3, k_p=1.0, **kw):
        a = dict(case, **kw)
        return L.hdsm_command_host(n, n_hor, step, dt, idx, k_p, a["n_ref"], a["ref_point"], a["state_before"], a["records"], a["valid"], a["state_after"],
                                   a["yaw"], None, pose, None)

    bad_valid, bad_yaw = case["valid"].copy(), case["yaw"].copy()
    bad_valid[3], bad_yaw[2] = 3, np.nan
    for kw in (dict(n=-1), dict(n_hor=0), dict(n_hor=17), dict(step=0), dict(step=11), dict(dt=0.0), dict(dt=np.inf), dict(dt=np.nan), dict(idx=-1),
               dict(idx=11), dict(k_p=np.nan), dict(k_p=np.inf), dict(n_ref=None), dict(ref_point=None), dict(state_before=None), dict(records=None),
               dict(valid=None), dict(state_after=None), dict(yaw=None), dict(valid=bad_valid), dict(yaw=bad_yaw)):
        assert rc(**kw) == lib.HDSM_ERR_BAD_ARG, kw
    assert not pose["valid"].any() and (case["yaw"] == keep).all()                                     # a refusal writes nothing
    assert rc(n=0, yaw=None, records=None) == 0 and rc(idx=10) == 0 and pose["valid"].any()
    with pytest.raises(lib.HdsmError) as e:
        lib.command(**dict(case, valid=bad_valid))
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: hdsm_command_host"
    # the mirror refuses the same settings, and every entry point a null handle
    shard = swarm.SwarmShard(agile_params(10), swarm.default_swarm_config(), 2, 0, np.zeros((2, 3)), np.ones((2, 3)))
    with pytest.raises(lib.HdsmError):
        shard.commands()                                                                              # before the first set_commands
    for kw in (dict(yaw_idx=-1), dict(yaw_idx=11), dict(k_p_yaw=np.nan), dict(yaw0=[0.0, np.inf])):
        with pytest.raises(lib.HdsmError):
            shard.set_commands(True, **kw)
    with pytest.raises(lib.HdsmError):
        shard.commands()
    shard.set_commands(True, yaw0=[0.25, -0.5])
    assert shard.commands()[2].tolist() == [0.25, -0.5] and not shard.commands()[1]["valid"].any()
    shard.set_commands(False)
    assert shard.commands()[2].tolist() == [0.25, -0.5]                                               # off keeps the yaw
    void = C.byref(C.c_void_p())
    for fn, args in (("hdsm_swarm_set_commands", (1, 3, 1.0, None)), ("hdsm_swarm_commands", (None, None, None)), ("hdsm_dswarm_set_commands", (1, 3, 1.0, None)),
                     ("hdsm_dswarm_commands", (None, None)), ("hdsm_dswarm_commands_device", (void, void)), ("hdsm_dswarm_command_stats", (np.zeros(3, np.int64),))):
        assert getattr(L, fn)(None, *args) == lib.HDSM_ERR_BAD_ARG, fn
    # the signatures come from the header
    f64, i32, i64, cmd, vpp = (lib.CTYPES[t] for t in ("double*", "int32_t*", "int64_t*", "hdsm_command*", "void**"))
    plain = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double, i32, f64, f64, f64, i32, f64, f64, cmd, cmd, i64]
    want = {"hdsm_command_host": plain, "hdsm_command_batch": [C.c_int32] + plain,
            "hdsm_swarm_set_commands": [C.c_void_p, C.c_int32, C.c_int32, C.c_double, f64], "hdsm_swarm_commands": [C.c_void_p, cmd, cmd, f64],
            "hdsm_dswarm_set_commands": [C.c_void_p, C.c_int32, C.c_int32, C.c_double, f64], "hdsm_dswarm_commands": [C.c_void_p, cmd, cmd],
            "hdsm_dswarm_commands_device": [C.c_void_p, vpp, vpp], "hdsm_dswarm_command_stats": [C.c_void_p, i64]}
    for name, argtypes in want.items():
        restype, got = lib.SIGNATURES[name]
        assert restype is C.c_int and got == argtypes and hasattr(L, name), name
    assert cmd.dtype == lib.COMMAND and lib.COMMAND.itemsize == 128 == C.sizeof(Command)
    assert [(n_, lib.COMMAND.fields[n_][1]) for n_ in lib.COMMAND.names] == [(n_, getattr(Command, n_).offset) for n_, _ in Command._fields_]
    assert (YAW_IDX, K_P_YAW) == (3, 1.0)


def _loop(oracle, prm):
    starts, goals = cc.exchange()

    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    return swarm.SwarmLoop(prm, swarm.default_swarm_config(), cc.N_FLIGHT, solve=solve, starts=starts, goals=goals)


def _view(loop, k, N):
    tr, pos, n_ref = np.zeros((N + 1, 3)), np.zeros(3), C.c_int32()
    P = C.POINTER(C.c_double)
    assert loop.shard.lib.hdsm_swarm_view(loop.shard.h, k, None, None, tr.ctypes.data_as(P), C.byref(n_ref), None, 0, None, None, None, None, None, None,
                                          pos.ctypes.data_as(P)) == 0
    return tr, pos, n_ref.value


def test_the_mirror_flight_against_the_libm_yaw(oracle):
    prm = agile_params(10, max_rows_static=18)
    N, n, step = prm.n_hor, cc.N_FLIGHT, swarm.default_swarm_config().step_plan
    mine, twin = _loop(oracle, prm), _loop(oracle, prm)
    mine.shard.set_commands(True)
    libm, prev = np.zeros(n), np.zeros(n)
    steps = wraps = fallbacks = 0
    worst = 0.0
    for r in range(cc.ROUNDS_FLIGHT):
        outs = []
        for loop in (mine, twin):
            inputs = loop.shard.prepare(loop.plans_all, loop.has_plan)
            outs.append(loop.solve(inputs, loop.plans_all, loop.has_plan))
        # the twin's yaw, where the reference computes it: after the solve, before the commit. No error may sit on the cut, where the last
        # bit of atan2 decides the direction of the wrap (the scenario's seed was picked on the CPU so that none does)
        for k in range(n):
            tr, pos, n_ref = _view(twin, k, N)
            v = tr[YAW_IDX] - pos
            if n_ref > YAW_IDX and v @ v > 0.1:
                err = math.atan2(v[1], v[0]) - prev[k]
                assert abs(abs(err) - math.pi) > 1e-9, (r, k, err)
                steps, wraps = steps + 1, wraps + (abs(err) > math.pi)
        assert twin.shard.lib.hdsm_swarm_yaw(twin.shard.h, YAW_IDX, K_P_YAW, libm) == 0
        prev = libm.copy()
        assert outs[0]["status"].tobytes() == outs[1]["status"].tobytes() and outs[0]["traj"].tobytes() == outs[1]["traj"].tobytes(), r
        for loop, out in zip((mine, twin), outs):
            loop.plans_all, loop.has_plan = loop.shard.commit(out)
        assert mine.plans_all.tobytes() == twin.plans_all.tobytes(), r                                  # commands do not steer
        sp, pose, yaw = mine.shard.commands()
        d = np.abs(yaw - libm)
        worst = max(worst, float(d.max()))
        assert (d <= 2 * cc.E + 8 * np.spacing(np.abs(libm))).all(), (r, yaw, libm)
        status, has = outs[0]["status"], mine.has_plan
        for k in range(n):
            want = 0 if not has[k] else (2 if status[k] == 2 else 1)
            assert pose[k]["valid"] == want and (sp[k]["valid"] == want).all(), (r, k)
            fallbacks += want == 2
            if want:
                for j in range(step):
                    knot = np.concatenate([sp[k, j]["pos"], sp[k, j]["vel"], sp[k, j]["acc"]])
                    assert knot.tobytes() == mine.plans_all[k, j + 1].tobytes(), (r, k, j)
                    assert sp[k, j]["yaw"] == yaw[k]
                assert np.concatenate([pose[k]["pos"], pose[k]["vel"], pose[k]["acc"]]).tobytes() == mine.plans_all[k, step].tobytes()
    # one more round in which the solver reports a failure for two agents: the shifted fallback is what they are told, marked 2
    inputs = mine.shard.prepare(mine.plans_all, mine.has_plan)
    out = mine.solve(inputs, mine.plans_all, mine.has_plan)
    out["status"][[1, 5]] = 2
    before = mine.plans_all.copy()
    mine.plans_all, mine.has_plan = mine.shard.commit(out)
    sp, pose, yaw = mine.shard.commands()
    assert pose["valid"].tolist() == [1, 2, 1, 1, 1, 2, 1, 1] and (sp[:, 0]["valid"] == pose["valid"]).all()
    for k in (1, 5):
        assert (mine.plans_all[k, :N] == before[k, 1:]).all()
        assert np.concatenate([sp[k, 0]["pos"], sp[k, 0]["vel"], sp[k, 0]["acc"]]).tobytes() == before[k, 2].tobytes()
    print(f"{cc.ROUNDS_FLIGHT} rounds: {steps} yaw steps, {wraps} through the wrap, {fallbacks} fallbacks, max |yaw - libm yaw| {worst:.3e}")
    assert steps > 4 * cc.ROUNDS_FLIGHT and np.abs(libm).max() > 0.5
