"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on seeded swarm snapshots.

Tolerances: the reference computes in IEEE double and Gurobi's own feasibility/optimality tolerances are
1e-6; BASELINE.json asks for trajectories within 1e-4. Both implementations here are exact active-set
solvers in fp64, so we demand much more: 1e-7 on trajectories/controls, 1e-6 relative on the objective.
"""
import numpy as np
import pytest

import problems
from enum_cases import enum_cases, enum_snapshot
from multi_agent_pkgs_amd.params import agile_params, default_params, make_params
from parity_cases import ARG_KEYS, FORCED_SHAPES, compare
from wave_cases import _mixed_batch

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    return lib


CASES = [
    dict(n_rob=16, seed=1),
    dict(n_rob=16, seed=2, turn=True),
    dict(n_rob=16, seed=3, narrow=True, turn=True),
    dict(n_rob=16, seed=4, spacing=1.0),
    dict(n_rob=16, seed=5, chamfer=True, narrow=True, turn=True),
    dict(n_rob=16, seed=6, first_round=True),
    dict(n_rob=64, seed=7, spacing=1.5, turn=True),
    dict(n_rob=64, seed=8, absent_frac=0.3),
    dict(n_rob=9, seed=9, narrow=True, chamfer=True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_replan_matches_oracle_h10(hdsm, oracle, case):
    prm = agile_params(10, max_rows_static=18)
    case = dict(case)
    n_rob = case.pop("n_rob")
    seed = case.pop("seed")
    sn = problems.swarm_snapshot(prm, n_rob, seed, **case)
    args = [sn[k] for k in ARG_KEYS]
    sol = hdsm.Solver(prm, n_rob, n_rob)
    g = sol.replan(*args)
    o = oracle.replan(prm, *args, n_threads=8)
    compare(g, o)


@pytest.mark.parametrize("n_hor,rk4,drag", [(15, False, (0, 0, 0)), (9, True, (0.1, 0.1, 0.3)), (12, True, (0, 0, 0)),
                                            (7, False, (0.2, 0.1, 0.0))])
def test_replan_matches_oracle_other_configs(hdsm, oracle, n_hor, rk4, drag):
    prm = agile_params(n_hor, max_rows_static=18, rk4=rk4, drag=drag)
    sn = problems.swarm_snapshot(prm, 25, seed=100 + n_hor, turn=True, narrow=(n_hor < 12))
    args = [sn[k] for k in ARG_KEYS]
    sol = hdsm.Solver(prm, 25, 25)
    g = sol.replan(*args)
    o = oracle.replan(prm, *args, n_threads=8)
    compare(g, o)


def test_default_config(hdsm, oracle):
    prm = default_params(9, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 20, seed=55, speed=(0, 4), turn=True)
    args = [sn[k] for k in ARG_KEYS]
    g = hdsm.Solver(prm, 20, 20).replan(*args)
    o = oracle.replan(prm, *args, n_threads=8)
    compare(g, o)


def test_tasc_planes_match_literal_chain(hdsm, oracle):
    """Trig-free closed form on the device vs the reference's acos/tan/atan/hypot chain (oracle)."""
    for r, h in [(0.25, 0.25), (0.25, 0.6), (0.125, 0.05)]:
        prm = agile_params(10, drone_radius=r, drone_z_offset=h)
        sn = problems.swarm_snapshot(prm, 12, seed=31, spacing=0.8)
        # vertical stacking exercises the ellipsoid term
        sn["plans"][3, :, :3] = sn["plans"][2, :, :3] + [0.0, 0.0, 0.9]
        sol = hdsm.Solver(prm, 12, 12)
        planes = sol.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"])
        for k in range(12):
            ref, valid = oracle.tasc_planes(prm, k, sn["state"][k], sn["plans"], sn["has_plan"])
            assert np.abs(planes[k] - ref).max() < 1e-12


def test_failed_instances_leave_outputs_untouched(hdsm):
    prm = agile_params(10, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 16, seed=4, spacing=1.0)
    args = [sn[k] for k in ARG_KEYS]
    sol = hdsm.Solver(prm, 16, 16)
    out = dict(traj=np.full((16, 11, 9), 7.0), ctrl=np.full((16, 10, 3), 7.0),
               used=np.full((16, 4), 7, dtype=np.uint8), status=np.zeros(16, dtype=np.int32), obj=np.full(16, 7.0))
    g = sol.replan(*args, out=out)
    bad = g["status"] == 2
    assert bad.any()
    assert (g["traj"][bad] == 7.0).all() and (g["ctrl"][bad] == 7.0).all() and (g["obj"][bad] == 7.0).all()


def test_capacity_and_argument_errors(hdsm):
    prm = agile_params(10)
    sol = hdsm.Solver(prm, 4, 8)
    sn = problems.swarm_snapshot(prm, 16, seed=1)
    with pytest.raises(hdsm.HdsmError) as e:
        sol.replan(*[sn[k] for k in ARG_KEYS])
    assert e.value.code == hdsm.HDSM_ERR_CAPACITY
    bad = agile_params(10)
    bad.r_u = 0.0
    with pytest.raises(hdsm.HdsmError) as e:
        hdsm.Solver(bad, 4, 4)
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(seed=41, narrow=True, turn=True, spacing=1.6), dict(seed=42, spacing=1.2)])
def test_level1_solve_matches_literal_oracle(hdsm, oracle, kw):
    """hdsm_solve (exact stand-in for the Gurobi call alone, AC:870-1019) on fully formed per-step polyhedra."""
    from multi_agent_pkgs_amd.params import make_params
    prm = make_params(n_hor=6, poly_hor=3, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 8, **kw)
    n_poly, n_rows, A, b = problems.level1_from_snapshot(
        prm, sn, lambda a: oracle.tasc_planes(prm, a, sn["state"][a], sn["plans"], sn["has_plan"]))
    g = hdsm.Solver(prm, 8, 8).solve(sn["state"], sn["ref"], n_poly, n_rows, A, b)
    o = oracle.solve(prm, sn["state"], sn["ref"], n_poly, n_rows, A, b, n_threads=8)
    compare(g, o)


@pytest.mark.parametrize("mstep", [1, 2])
def test_rows_on_input_independent_positions_are_judged_with_feas_tol_fixed(hdsm, oracle, mstep):
    """Under Euler p_1 and p_2 do not depend on the inputs: a row there is a constant, judged like a row on the pinned p_0 —
    violated by 1e-8 or 1e-7 it holds (Gurobi's FeasibilityTol 1e-6, hdsm_params.feas_tol_fixed) and the optimum is the one
    without the row; violated by 1e-5 nothing can satisfy it (AC:988-1019: the caller falls back)."""
    from multi_agent_pkgs_amd.params import make_params
    prm = make_params(n_hor=8, poly_hor=2, max_rows_static=18)
    sol = hdsm.Solver(prm, 1, 1)
    base = None
    for delta, want in ((-1.0, 0), (1e-8, 0), (1e-7, 0), (1e-5, 2)):
        args = problems.constant_row_case(prm, oracle, mstep, delta)
        g, o = sol.solve(*args), oracle.solve(prm, *args)
        assert g["status"][0] == want and o["status"][0] == want, (mstep, delta, g["status"], o["status"])
        if want == 0:
            compare(g, o)
            base = g["traj"].copy() if base is None else base
            assert np.abs(g["traj"] - base).max() < 1e-9, (mstep, delta)   # the row that holds within the tolerance changes nothing


def test_closed_loop_on_device_matches_oracle_loop(hdsm, oracle):
    """20 closed-loop rounds of an 8-agent circle exchange: device solver vs oracle solver, same host code."""
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    sol = hdsm.Solver(prm, 8, 8)

    def dev(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    la = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 8, solve=dev)
    lb = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 8, solve=cpu)
    for r in range(45):
        la.step()
        lb.step()
    assert np.abs(la.plans_all - lb.plans_all).max() < 1e-6


def test_warm_start_never_changes_the_answer(hdsm, oracle):
    """The previous working set only seeds the dual method. Feeding a handle unrelated problems back to back
    (a deliberately WRONG guess) must still give the oracle's optimum; so must a second solve of the same
    problem (a perfect guess), in fewer iterations."""
    prm = agile_params(10, max_rows_static=18)
    sol = hdsm.Solver(prm, 25, 25)
    cold = hdsm.Solver(agile_params(10, max_rows_static=18, warm_start=False), 25, 25)
    first = None
    for seed, kw in [(61, dict(spacing=1.2)), (62, dict(turn=True, spacing=1.0)), (61, dict(spacing=1.2)), (61, dict(spacing=1.2))]:
        sn = problems.swarm_snapshot(prm, 25, seed, **kw)
        args = [sn[k] for k in ARG_KEYS]
        g = sol.replan(*args)
        o = oracle.replan(prm, *args, n_threads=8)
        compare(g, o)
        gc = cold.replan(*args)
        compare(gc, o)
        if first is None:
            first = gc["qp_iters"].copy()
    # last call repeated the same problem: its own working sets were the guess (shifted by one step as for the next
    # replan, so not a perfect hit). The count includes the operations that install the guess (one per row, cheaper than a
    # regular iteration: no scan, no step), and with the normalised pick rule a cold start needs about as many iterations as
    # the final working set has rows — so this is only a sanity bound; the closed-loop test below measures the time.
    assert g["qp_iters"].sum() <= 2.5 * gc["qp_iters"].sum()


def test_warm_start_closed_loop_is_the_same_flight_in_less_kernel_time(hdsm):
    from multi_agent_pkgs_amd import swarm
    res = {}
    for warm in (False, True):
        prm = agile_params(10, max_rows_static=18, warm_start=warm)
        sol = hdsm.Solver(prm, 32, 32)
        sol.set_kernel_timing(True)
        its, ms = [], []

        def dev(inp, plans, has):
            out = sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)
            its.append(out["qp_iters"].max())
            ms.append(sol.last_kernel_ms())
            return out

        loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 32, solve=dev)
        for r in range(60):
            loop.step()
        res[warm] = (np.array(its), loop.plans_all.copy(), np.array(ms))
    assert np.abs(res[True][1] - res[False][1]).max() < 1e-6        # same flight
    print("rounds 20..59, cold vs warm: operations of the slowest instance", res[False][0][20:60].mean(), res[True][0][20:60].mean(),
          "kernel ms per round", res[False][2][20:60].mean(), res[True][2][20:60].mean())
    assert res[True][2][20:60].sum() < 1.05 * res[False][2][20:60].sum()


@pytest.mark.parametrize("n_rob,n_hor", [(256, 10), (128, 15)])
def test_full_size_properties(hdsm, oracle, n_rob, n_hor):
    """BASELINE-scale batch (256 agents H=10 / 128 agents H=15, every agent sees every other agent's planes):
    size-independent properties on ALL instances + oracle parity on a random subset.
      * the trajectory is the literal rollout of the returned controls (dynamics AC:2115-2167),
      * input / velocity / acceleration boxes and the terminal v_N = a_N = 0 hold (AC:2078-2084, 2179-2186),
      * every separating plane of every step holds at p_i and p_{i+1} (AC:909-941 + AC:1086-1215),
      * every segment lies in a polyhedron flagged in poly_used (AC:979-985),
      * obj is the literal objective (AC:870-883)."""
    prm = agile_params(n_hor, max_rows_static=18)
    N = n_hor
    sn = problems.swarm_snapshot(prm, n_rob, seed=500 + n_rob, spacing=1.8, turn=True)
    args = [sn[k] for k in ARG_KEYS]
    sol = hdsm.Solver(prm, n_rob, n_rob)
    g = sol.replan(*args)
    ok = np.where(g["status"] == 0)[0]
    assert len(ok) > n_rob // 2
    planes = sol.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"])  # [inst][N][n_rob][4]
    pinned = 0 if prm.rk4 else 2  # p_0 .. p_pinned do not depend on the inputs: rows there are judged with feas_tol_fixed
    for a in ok:
        traj, ctrl = g["traj"][a], g["ctrl"][a]
        assert np.abs(oracle.rollout(prm, sn["state"][a], ctrl) - traj).max() < 1e-10
        assert np.abs(ctrl).max() <= 60 + 1e-8
        assert np.abs(traj[1:N, 3:6]).max() <= 20 + 1e-8 and np.abs(traj[1:N, 6:9]).max() <= 15 + 1e-8
        assert np.abs(traj[N, 3:9]).max() < 1e-8
        assert abs(oracle.objective(prm, traj, ctrl, sn["ref"][a]) - g["obj"][a]) < 1e-7 * max(1, abs(g["obj"][a]))
        for i in range(N):
            rows = planes[a, i]
            for m in (i, i + 1):
                viol = (rows[:, :3] @ traj[m, :3] - rows[:, 3]).max()
                assert viol < (1e-6 if m <= pinned else 1e-7), (a, i, m, viol)
            inside = [j for j, (A, b) in enumerate(sn["polys"][a][: prm.poly_hor]) if g["used"][a, j]
                      and (A @ traj[i, :3] - b).max() < (1e-6 if i <= pinned else 1e-7)
                      and (A @ traj[i + 1, :3] - b).max() < (1e-6 if i + 1 <= pinned else 1e-7)]
            assert inside, (a, i)
    rng = np.random.default_rng(0)
    sub = rng.choice(n_rob, 24, replace=False)
    o = oracle.replan(prm, sn["agent_id"][sub], sn["state"][sub], sn["ref"][sub], sn["n_poly"][sub], sn["n_rows"][sub],
                      sn["A"][sub], sn["b"][sub], sn["plans"], sn["has_plan"], n_threads=8)
    compare({k: g[k][sub] for k in ("status", "traj", "ctrl", "obj")}, o)


def test_reference_kernel_matches_oracle(hdsm, oracle):
    """Row f1 on the device vs its oracle: exp/pow differ from glibc by an ulp or two -> 1e-10 relative."""
    from multi_agent_pkgs_amd.params import agile_ref_config
    rng = np.random.default_rng(5)
    # (16, ...): the last step of the longest horizon (second slot of lane 0 in k_ref_pack); 1500 agents in two far clusters:
    # the sphere cull of the velocity limit skips most neighbours; sens_dist < 0: the limit is not monotone in the distance
    # and every pair is evaluated
    for n_hor, n_rob, sens_other, sens_dist in [(10, 64, 1.0, None), (15, 200, 0.8, None), (7, 9, 1.0, None), (16, 300, 0.9, None),
                                                (10, 1500, 1.0, None), (10, 130, 1.0, -0.2)]:
        prm = agile_params(n_hor, max_rows_static=18)
        kw = {} if sens_dist is None else {"sens_dist": sens_dist}
        rcfg = agile_ref_config(sens_other_agents=sens_other, path_vel_dec=0.5 if n_hor == 7 else 0.0, **kw)
        sn = problems.swarm_snapshot(prm, n_rob, seed=70 + n_hor, spacing=1.5)
        if n_rob == 1500:  # second cluster 400 m away
            sn["plans"][750:, :, 0] += 400.0
            sn["state"][750:, 0] += 400.0
        sn["has_plan"][rng.random(n_rob) < 0.1] = 0
        path = np.zeros((n_rob, 3, 3))
        n_path = np.full(n_rob, 3, np.int32)
        for k in range(n_rob):
            p0 = sn["state"][k, :3]
            path[k] = [p0, p0 + rng.normal(size=3) * [2, 2, 0.2], p0 + rng.normal(size=3) * [6, 6, 0.3]]
        n_path[::7] = 2
        n_path[3] = 1
        cap = rng.uniform(5.0, 12.0, n_rob)
        sol = hdsm.Solver(prm, n_rob, n_rob)
        for vc in (None, cap):
            g = sol.reference(rcfg, sn["agent_id"], path, n_path, sn["plans"], sn["has_plan"], vel_cap=vc)
            o = oracle.reference(prm, rcfg, sn["agent_id"], path, n_path, sn["plans"], sn["has_plan"], vel_cap=vc)
            for x, y in zip(g, o):
                assert np.abs(x - y).max() < 1e-10 * max(1.0, np.abs(y).max())
        assert (o[2][n_path >= 2] <= 9.0 + 1e-12).all() and o[2][3] == 0.0


def test_closed_loop_with_device_reference(hdsm, oracle):
    """Solver AND reference generation on the device vs the all-host/oracle loop."""
    from multi_agent_pkgs_amd import swarm
    from multi_agent_pkgs_amd.params import agile_ref_config
    prm = agile_params(10, max_rows_static=18)
    rcfg = agile_ref_config()
    sol = hdsm.Solver(prm, 12, 12)

    def dev(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def dev_ref(ids, path, n_path, plans, has):
        full, ref, pv = sol.reference(rcfg, ids, path, n_path, plans, has)
        return full, pv

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    la = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 12, solve=dev, reference=dev_ref)
    lb = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 12, solve=cpu)
    for r in range(40):
        la.step()
        lb.step()
    assert np.abs(la.plans_all - lb.plans_all).max() < 1e-6


@pytest.mark.parametrize("case", [dict(n_rob=64, seed=7, spacing=1.5, turn=True), dict(n_rob=64, seed=8, absent_frac=0.3),
                                  dict(n_rob=16, seed=6, first_round=True), dict(n_rob=100, seed=11, spacing=6.0)],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_sphere_prefilter_never_changes_the_answer(hdsm, oracle, case, monkeypatch):
    """Sweeps that first skip whole neighbours by bounding spheres (k_plan_bounds, default for >= 256 agents; forced
    here by HDSM_BOUNDS_MIN=1) stage exactly the rows the step-by-step test would: same result as without it and
    as the oracle, which generates every plane (AC:1100-1205)."""
    prm = agile_params(10, max_rows_static=18)
    case = dict(case)
    n_rob, seed = case.pop("n_rob"), case.pop("seed")
    sn = problems.swarm_snapshot(prm, n_rob, seed, **case)
    args = [sn[k] for k in ARG_KEYS]
    monkeypatch.setenv("HDSM_BOUNDS_MIN", "1")
    g_pre = hdsm.Solver(prm, n_rob, n_rob).replan(*args)
    monkeypatch.setenv("HDSM_BOUNDS_MIN", "1000000")
    g_all = hdsm.Solver(prm, n_rob, n_rob).replan(*args)
    assert (g_pre["status"] == g_all["status"]).all()
    ok = g_all["status"] != 2
    assert np.abs(g_pre["traj"] - g_all["traj"])[ok].max() < 1e-9
    compare(g_pre, oracle.replan(prm, *args, n_threads=8))


@pytest.mark.parametrize("bad", [np.inf, "both"], ids=["plus-inf", "plus-and-minus-inf"])
def test_sphere_prefilter_keeps_the_finite_steps_of_a_non_finite_plan(hdsm, oracle, monkeypatch, bad):
    """A neighbour S with has_plan = 1 whose x coordinate is +inf at the last two steps (the centre of its sphere is infinite), or
    +inf at the last step and -inf at the one before (the centre is NaN): its record is the never-culled one (radius 1e300), and
    the sphere prefilter (forced by HDSM_BOUNDS_MIN=1) must list it, because the planes of its finite steps shape the answer.
    S is the first agent for which they do: the oracle's answer for some other agent moves by more than 1e-3 m when S's
    has_plan is cleared. The kernel against the oracle on the plans as published, tolerances of compare()."""
    prm = agile_params(10, max_rows_static=18)
    n_rob, N = 16, prm.n_hor
    sn = problems.swarm_snapshot(prm, n_rob, seed=2, turn=True)
    head = [sn[k] for k in ARG_KEYS[:-2]]
    for S in range(n_rob):
        plans, gone = sn["plans"].copy(), sn["has_plan"].copy()
        plans[S, N - 1:, 0] = np.inf
        if bad == "both":
            plans[S, N - 1, 0] = -np.inf
        gone[S] = 0
        want = oracle.replan(prm, *head, plans, sn["has_plan"], n_threads=8)
        without = oracle.replan(prm, *head, plans, gone, n_threads=8)
        others = (np.arange(n_rob) != S) & (want["status"] == 0) & (without["status"] == 0)
        if sn["has_plan"][S] and others.any() and np.abs(want["traj"] - without["traj"])[others].max() > 1e-3:
            break
    else:
        raise AssertionError("no agent whose finite steps decide another agent's answer")
    monkeypatch.setenv("HDSM_BOUNDS_MIN", "1")
    sol = hdsm.Solver(prm, n_rob, n_rob)
    g = sol.replan(*head, plans, sn["has_plan"])
    assert (sol.last_sweep_stats(n_rob)["sphere_records"] > 0).any()      # the sphere list ran
    assert (want["status"] == 0).sum() > n_rob // 2
    compare(g, want)
    sol.close()


def test_sphere_prefilter_chunks_beyond_list_capacity(hdsm, oracle):
    """1300 agents (> one chunk of 1024 neighbours): instances from both ends of the id range against the oracle."""
    prm = agile_params(10, max_rows_static=18)
    n_rob = 1300
    sn = problems.swarm_snapshot(prm, n_rob, seed=77, spacing=1.7, turn=True)
    sub = np.concatenate([np.arange(0, 20), np.arange(1010, 1040), np.arange(1280, 1300)]).astype(np.int32)
    sel = [sn[k][sub] for k in ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")] + [sn["plans"], sn["has_plan"]]
    g = hdsm.Solver(prm, len(sub), n_rob).replan(*sel)
    o = oracle.replan(prm, *sel, n_threads=8)
    assert (o["status"] == 0).sum() > len(sub) // 2
    compare(g, o)


def test_maximum_dimensions(hdsm, oracle):
    """The largest shapes the ABI admits (HDSM_MAX_HOR = 16, HDSM_MAX_POLY = 8, HDSM_MAX_ROWS_STATIC = 32): ragged
    n_poly (2..4 of 8 slots used), static polyhedra padded to 30 rows with positive multiples of their own rows
    (same feasible set, linearly dependent normals), absent neighbours."""
    prm = agile_params(16, poly_hor=8, max_rows_static=32)
    sn = problems.swarm_snapshot(prm, 16, seed=906, spacing=1.5, box_half=5.0, absent_frac=0.2)
    polys = []
    for plist in sn["polys"]:
        out = []
        for A, b in plist:
            rows_A, rows_b, k = [A], [b], 2.0
            while sum(len(x) for x in rows_b) + len(b) <= 30:
                rows_A.append(k * A), rows_b.append(k * b)
                k += 1.0
            out.append((np.vstack(rows_A), np.concatenate(rows_b)))
        polys.append(out)
    n_poly, n_rows, A, b = problems.pack_static(polys, prm.poly_hor, prm.max_rows_static)
    assert n_rows.max() == 30 and n_poly.min() < n_poly.max() <= 8
    args = [sn["agent_id"], sn["state"], sn["ref"], n_poly, n_rows, A, b, sn["plans"], sn["has_plan"]]
    g = hdsm.Solver(prm, 16, 16).replan(*args)
    o = oracle.replan(prm, *args, n_threads=8)
    assert (o["status"] == 0).sum() >= 6
    compare(g, o)


def test_empty_batch_is_a_no_op(hdsm):
    prm = agile_params(10)
    sol = hdsm.Solver(prm, 4, 8)
    sn = problems.swarm_snapshot(prm, 8, seed=3)
    sel = [sn[k][:0] for k in ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")] + [sn["plans"], sn["has_plan"]]
    g = sol.replan(*sel)
    assert g["traj"].shape[0] == 0 and g["status"].shape[0] == 0


def test_baseline_config_1_single_agent(hdsm, oracle):
    """BASELINE configs[0]: ONE agent, start (0, 0, 1.5), goal (42.15, 42.15, 1.5) (agent_agile_config.yaml:42-43),
    empty world, H = 10: a chain of up to four overlapping free-space boxes, so the problem is a genuine MIQP although
    there are no neighbours. Closed loop on the device against the same loop on the oracle."""
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    sol = hdsm.Solver(prm, 1, 1)
    start, goal = [[0.0, 0.0, 1.5]], [[42.15, 42.15, 1.5]]
    used_max = [0]

    def dev(inp, plans, has):
        out = sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)
        used_max[0] = max(used_max[0], int(out["used"].sum()))
        return out

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    la = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 1, solve=dev, starts=start, goals=goal)
    lb = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 1, solve=cpu, starts=start, goals=goal)
    for r in range(60):
        oa, ob = la.step(), lb.step()
        assert oa["status"][0] == ob["status"][0] == 0, r
    assert np.abs(la.plans_all - lb.plans_all).max() < 1e-6
    pos, dist, nfail = la.shard.state()
    assert nfail[0] == 0 and dist[0] < 35.0  # 59.6 m to go at the start; moving at 4.5..9 m/s for 6 s
    assert used_max[0] >= 2                   # several polyhedra in use on one horizon: the binaries matter


def test_closed_loop_through_a_forest_with_voxel_corridors(hdsm, oracle):
    """Next row f2 end to end: 12 agents in line formation fly through a pillar forest; every round the host cuts the
    local voxel grids out of the world, decomposes them (hdsm_poly_octa3d) into chamfered polyhedra, and the device
    solves. Same loop on the oracle; nobody touches an occupied voxel."""
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    starts, goals, occ, origin = swarm.lane_forest_scenario(6, 2, seed=1)
    sol = hdsm.Solver(prm, 12, 12)
    rows_max = [0]

    def dev(inp, plans, has):
        rows_max[0] = max(rows_max[0], int(inp["n_rows"].max()))
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    la = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 12, solve=dev, starts=starts, goals=goals)
    lb = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 12, solve=cpu, starts=starts, goals=goals)
    la.shard.set_world(occ, origin), lb.shard.set_world(occ, origin)
    for r in range(70):
        oa, ob = la.step(), lb.step()
        assert (oa["status"] == ob["status"]).all(), r
        pos, _, _ = la.shard.state()
        ij = np.floor((pos - origin) / 0.3).astype(int)
        assert not (occ[ij[:, 2], ij[:, 1], ij[:, 0]] >= 100).any(), r
    assert np.abs(la.plans_all - lb.plans_all).max() < 1e-6
    assert rows_max[0] > 6                      # chamfered polyhedra were in play
    assert la.shard.state()[0][:, 0].min() > 25  # and the formation is through most of the first forest band


@pytest.mark.parametrize("cfgkw,shape", [
    (dict(), (3, 20, 66, 66)),                                                   # the local grid of the reference, shipped parameters
    (dict(inflation_dist=0.6, potential_dist=1.2, potential_pow=2), (2, 17, 33, 41)),
    (dict(voxel_size=0.2, inflation_dist=0.3, potential_dist=1.0, potential_pow=3), (2, 9, 50, 23)),
    (dict(inflation_dist=0.0, potential_dist=0.9, potential_pow=1), (1, 8, 30, 30)),
])
def test_map_preprocess_matches_the_literal_loops(hdsm, oracle, cfgkw, shape):
    """Next row f4, bit-exact: the device's distance-transform formulation of SetUncertainToUnknown / InflateObstacles /
    CreatePotentialField against the oracle's literal scatter loops, on random worlds with pillars, walls, unknown
    regions and obstacles on the borders."""
    from multi_agent_pkgs_amd.params import default_map_config
    cfg = default_map_config(**cfgkw)
    rng = np.random.default_rng(hash(shape) % 1000)
    g = np.zeros(shape, np.int8)
    n, nz, ny, nx = shape
    for b in range(n):
        for _ in range(int(rng.integers(3, 40))):
            x, y = int(rng.integers(0, nx)), int(rng.integers(0, ny))
            g[b, : int(rng.integers(1, nz + 1)), y, x] = 100
        g[b, int(rng.integers(0, nz)), :, int(rng.integers(0, nx))] = 100           # a beam
        unk = rng.random((nz, ny, nx)) < 0.02
        g[b][unk & (g[b] == 0)] = -1                                                 # scattered unknown voxels
        g[b, :, : ny // 5, : nx // 4][g[b, :, : ny // 5, : nx // 4] == 0] = -1       # an unexplored corner
    dev = hdsm.map_preprocess(cfg, g)
    ref = oracle.map_preprocess(cfg, g)
    assert dev.dtype == np.int8 and (dev == ref).all(), int((dev != ref).sum())
    assert ((ref > 0) & (ref < 100)).any() and (ref == -1).any()
    assert (ref == 100).sum() > (g == 100).sum() or cfg.inflation_dist == 0


def test_cpp_example_runs_the_closed_loop_through_the_c_abi():
    """examples/closed_loop.cpp: the ABI driven from C++ with no Python in between (built by `make -C examples`)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s"])
    out = subprocess.run([os.path.join(root, "examples", "closed_loop"), "12", "110"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    line = out.stdout.strip()
    assert "12 agents, 110 rounds" in line
    sep = float(line.split("closest approach ")[1].split(" m")[0])
    far = float(line.split("farthest agent ")[1].split(" m")[0])
    assert sep > 0.45 and far < 2.0, line   # separation planes keep the 0.25 m-radius drones apart; everybody crossed the 44 m circle


def test_map_preprocess_edge_cases(hdsm, oracle):
    """Tiny grids (every voxel next to a border, quads running over the ends of rows and of the buffer), an empty batch,
    a batch of one-voxel-thick slabs, and the rejection of masks wider than the byte-sized distance field."""
    from multi_agent_pkgs_amd.params import default_map_config
    cfg = default_map_config()
    rng = np.random.default_rng(3)
    for shape in [(2, 3, 5, 7), (3, 1, 9, 9), (1, 6, 1, 13), (4, 2, 2, 3), (1, 11, 13, 1)]:
        g = np.zeros(shape, np.int8)
        g[rng.random(shape) < 0.06] = 100
        g[(rng.random(shape) < 0.05) & (g == 0)] = -1
        assert (hdsm.map_preprocess(cfg, g) == oracle.map_preprocess(cfg, g)).all(), shape
    assert hdsm.map_preprocess(cfg, np.zeros((0, 4, 4, 4), np.int8)).shape == (0, 4, 4, 4)
    with pytest.raises(hdsm.HdsmError) as e:
        hdsm.map_preprocess(default_map_config(potential_dist=3.5), np.zeros((1, 4, 4, 4), np.int8))  # rn = 12 > 9
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG


def test_enumerated_miqp_goldens_on_the_device(hdsm):
    """tests/golden/miqp_enum.npz — six N = 6 / P = 3 cases with all 729 assignments resolved, three N = 10 / P = 4 cases with every
    admissible assignment resolved (scipy + KKT certificates + LP infeasibility proofs; planes from refmath, not from the
    oracle): the device must return the enumerated optimum. Objective to 1e-6 relative, trajectory to 1e-4 (the tolerance
    BASELINE.json states against the reference solve) where the optimum is unique."""
    import refmath as rm
    n = 0
    for k, c in enum_cases():
        prm, polys, args = enum_snapshot(c)
        sol = hdsm.Solver(prm, 1, args[7].shape[0])
        for rep in range(2):   # cold, then warm-started from its own answer
            g = sol.replan(*args)
            want = float(c["obj"])
            assert g["status"][0] == 0 and abs(g["obj"][0] - want) < 1e-6 * max(1.0, abs(want)), (k, rep, g["obj"], want)
            if float(c["second"]) - want > 1e-3 * max(1.0, abs(want)):
                assert np.abs(g["traj"][0] - rm.rollout(prm, c["state"], c["u"])).max() < 1e-4, (k, rep)
            used = set(np.where(g["used"][0])[0].tolist())
            assert used == set(c["leaf_assign"][0].tolist()) or float(c["second"]) - want <= 1e-3 * max(1.0, abs(want)), (k, used)
        sol.close()
        n += 1
    assert n >= 9


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_subtree_splitting_gives_the_unsplit_answer(hdsm, oracle, depth, monkeypatch):
    """The split launch forced on (HDSM_SPLIT=1) with a two-node budget: every instance that branches is handed over to
    poly_hor^depth sub-blocks (shared incumbent, merge kernel). Same answers as the one-kernel launch and as the oracle, on
    corridors that force real branching and on the enumerated MIQP goldens (where the optimum is certified independently)."""
    prm = agile_params(10, max_rows_static=18)
    plain_sol = hdsm.Solver(prm, 10, 10)
    monkeypatch.setenv("HDSM_SPLIT", "1")
    monkeypatch.setenv("HDSM_SPLIT_BUDGET", "2")
    monkeypatch.setenv("HDSM_SPLIT_DEPTH", str(depth))
    sol = hdsm.Solver(prm, 10, 10)
    handed = 0
    for seed in (3, 5, 21):
        sn = problems.swarm_snapshot(prm, 10, seed, narrow=True, turn=True, chamfer=(seed % 2 == 1))
        args = [sn[k] for k in ARG_KEYS]
        for rep in range(2):   # cold, then warm-started
            g, p = sol.replan(*args), plain_sol.replan(*args)
            compare(g, oracle.replan(prm, *args, n_threads=8))
            assert np.array_equal(g["status"], p["status"]) and np.abs(g["traj"] - p["traj"]).max() < 1e-9
        handed += int((p["nodes"] > 2).sum())
    assert handed >= 3
    sol.close()
    for k, c in enum_cases():
        eprm, polys, args = enum_snapshot(c)
        es = hdsm.Solver(eprm, 1, args[7].shape[0])
        g = es.replan(*args)
        want = float(c["obj"])
        assert g["status"][0] == 0 and abs(g["obj"][0] - want) < 1e-6 * max(1.0, abs(want)), (k, g["obj"], want, g["nodes"])
        es.close()


def test_pick_rule_changes_the_path_not_the_answer(hdsm, oracle, monkeypatch):
    """HDSM_PICK_RULE = 0 (most violated row first) and 1 (most violated in the metric of the problem, the default): two paths of
    the dual method to the same optimum — same statuses, same trajectories, on plain, turning and branching corridors and on an
    infeasible batch (agents far above the velocity limit); the default needs no more operations in total."""
    prm = agile_params(10, max_rows_static=18)
    monkeypatch.setenv("HDSM_PICK_RULE", "0")
    raw = hdsm.Solver(prm, 25, 25)
    monkeypatch.setenv("HDSM_PICK_RULE", "1")
    nrm = hdsm.Solver(prm, 25, 25)
    ops = [0, 0]
    for seed, kw in [(71, dict(spacing=1.2)), (72, dict(turn=True, spacing=1.0)), (73, dict(narrow=True, turn=True)), (74, dict(spacing=0.8))]:
        sn = problems.swarm_snapshot(prm, 25, seed, **kw)
        if seed == 74:
            sn["state"] = sn["state"].copy()
            sn["state"][::3, 3] = 40.0
        args = [sn[k] for k in ARG_KEYS]
        o = oracle.replan(prm, *args, n_threads=8)
        for k, sol in enumerate((raw, nrm)):
            g = sol.replan(*args)
            compare(g, o)
            ops[k] += int(g["qp_iters"].sum())
    print("operations, raw rule vs normalised rule:", ops)
    assert ops[1] <= ops[0]


def test_the_set_up_map_on_the_matrix_cores_gives_the_answers_of_the_per_instance_form(hdsm, oracle, monkeypatch):
    """Round 5: everything an instance needs before its first iteration is linear in (state_curr, traj_ref); the pre-pass kernel now
    applies that map to ALL instances of a launch as one dense product through v_mfma_f64_16x16x4_f64 (hdsm_api.hip, setup_map_tile)
    and the solver reads one number per thread. HDSM_SETUP_MFMA=0 keeps the per-instance form of rounds 1-4 (a 23-term dot product per
    thread): same statuses, trajectories equal to rounding, both equal to the oracle — at H = 10 and at H = 15 (147 outputs per
    instance: more than a 128-thread workgroup has threads), with a batch that is not a multiple of the 16-instance tile."""
    for N, n_inst, seed in ((10, 37, 3), (15, 21, 4)):
        prm = agile_params(N, max_rows_static=18)
        sn = problems.swarm_snapshot(prm, n_inst, seed=seed, spacing=1.2, turn=True, narrow=True)
        args = [sn[k] for k in ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")]
        monkeypatch.setenv("HDSM_SETUP_MFMA", "0")
        plain = hdsm.Solver(prm, n_inst, n_inst).replan(*args)
        monkeypatch.setenv("HDSM_SETUP_MFMA", "1")
        mfma = hdsm.Solver(prm, n_inst, n_inst).replan(*args)
        monkeypatch.delenv("HDSM_SETUP_MFMA")
        o = oracle.replan(prm, *args, n_threads=8)
        assert (mfma["status"] == plain["status"]).all() and (mfma["status"] == o["status"]).all()
        ok = o["status"] != 2
        assert ok.any()
        assert np.abs(mfma["traj"] - plain["traj"])[ok].max() < 1e-9
        assert np.abs(mfma["traj"] - o["traj"])[ok].max() < 1e-7
        assert (np.abs(mfma["obj"] - o["obj"])[ok] / np.maximum(1.0, np.abs(o["obj"][ok]))).max() < 1e-6


@pytest.mark.parametrize("shape", list(FORCED_SHAPES))
def test_every_launch_shape_matches_the_oracle(hdsm, oracle, monkeypatch, shape):
    """Each of the eight k_replan* launch shapes (tests/test_wave_shapes.py: the same batches through their CPU execution) picked on
    purpose for one batch that narrows, turns, is chamfered and has neighbours without a plan — until now only the fuzz reached some
    of them, by chance."""
    import staging_cases as sc
    n_hor, threads, env = FORCED_SHAPES[shape]
    prm = make_params(n_hor=n_hor, max_rows_static=18, poly_hor=4, threads_per_instance=threads)
    args = _mixed_batch(prm, 16, 310 if n_hor == 10 else 317, every=2 if n_hor == 10 else 4)
    o = sc.verdict(oracle, prm, args, n_threads=32)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    sol = hdsm.Solver(prm, args[1].shape[0], args[7].shape[0])
    for k_ in env:
        monkeypatch.delenv(k_)
    g = sol.replan(*args)
    assert (g["status"] == o["status"]).all(), (g["status"], o["status"])
    ok = o["status"] == 0
    assert ok.any() and np.abs(g["traj"] - o["traj"])[ok].max() < 1e-6
    assert (np.abs(g["obj"] - o["obj"])[ok] / np.maximum(1, np.abs(o["obj"][ok]))).max() < 1e-8
