"""Plan shifts and the own-plan override of the solver handle on the MI355X (hdsm_set_plan_shift, hdsm_set_plan_shift_device,
hdsm_set_own_plans_device; include/hdsm.h) on the cases of tests/shift_cases.py: 16 agents at H = 7 / 10 / 15, shifts 0, 1, N - 1, N,
N + 3 and ages times step_plan (1 and 3), two agents without a plan. The yardstick is the oracle called per instance on
materialised records; tests/test_plan_shift.py asserts on the CPU that those answers differ from the unshifted ones.

Tolerances: statuses equal, trajectories 1e-7, objective 1e-6 relative (tests/test_gpu_parity.py); the reference row 1e-10 relative
(tests/test_gpu_reference_row.py); planes 1e-12 (tests/test_gpu_groups.py)."""
import numpy as np
import pytest

import shift_cases as sc
from parity_cases import compare, stale_outputs

pytestmark = pytest.mark.gpu
ARG_KEYS = sc.ARG_KEYS


@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    return lib


def _device_replan(sol, c, sn_args, dev):
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in zip(ARG_KEYS, sn_args)}
    o = stale_outputs(sc.N_ROB, c.n_hor, c.prm().poly_hor, dev)
    torch.cuda.synchronize()
    sol.replan_device(*[d[k] for k in ARG_KEYS], o["traj"], o["ctrl"], o["used"], o["status"], o["obj"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("prefilter", [1, -1], ids=["prefilter", "no-prefilter"])
@pytest.mark.parametrize("idx", range(len(sc.CASES)), ids=sc.IDS)
def test_shifted_replan_matches_the_oracle_on_materialised_records(hdsm, oracle, idx, prefilter):
    """hdsm_replan (host arrays) and hdsm_replan_device (k_plan_prepass on device arrays, the shift as a host array and as a borrowed
    device array), with the sphere prefilter on at this size (prefilter_min_agents = 1) and off; twice on one handle, so that the second
    call rebuilds its warm-start rows from the shifted positions. Cleared, the handle answers as one that never had a shift."""
    import torch
    c = sc.case(idx)
    prm = c.prm(prefilter_min_agents=prefilter)
    want, plain = c.want(oracle, "shifted"), c.want(oracle, "unshifted")
    dev = torch.device("cuda", 0)
    sol = hdsm.Solver(prm, sc.N_ROB, sc.N_ROB)
    sol.set_plan_shift(c.shift)
    for rep in range(2):
        compare(sol.replan(*c.args()), want)
    if prefilter > 0:
        assert (sol.last_sweep_stats(sc.N_ROB)["sphere_records"] > 0).any()
    sol.reset_warm_start()
    compare(_device_replan(sol, c, c.args(), dev), want)
    d_shift = torch.from_numpy(c.shift).to(dev)
    sol.set_plan_shift_device(d_shift)                     # replaces the host form; entries above N behave as N here too
    sol.reset_warm_start()
    compare(_device_replan(sol, c, c.args(), dev), want)
    d_shift.zero_()                                        # borrowed: read at each launch
    torch.cuda.synchronize()
    sol.reset_warm_start()
    compare(_device_replan(sol, c, c.args(), dev), plain)
    sol.set_plan_shift_device(None)
    sol.set_plan_shift(c.shift)
    sol.set_plan_shift(None)
    sol.reset_warm_start()
    compare(sol.replan(*c.args()), plain)
    sol.close()


@pytest.mark.parametrize("idx", [1, 2, 5], ids=[sc.IDS[1], sc.IDS[2], sc.IDS[5]])
def test_own_plan_override(hdsm, oracle, idx):
    """The own slots of plans_all hold a decoy, the true records come through hdsm_set_own_plans_device; agent 5 has no plan for the
    others (has_plan 0) and flies its own (own_has 1). With d_own_has NULL the own flag stays has_plan: agent 5 then starts from its
    state, as the oracle does when its flag is 0 and its record the true one."""
    import torch
    c = sc.case(idx)
    dev = torch.device("cuda", 0)
    want = c.want(oracle, "override")
    d_own, d_has = torch.from_numpy(np.ascontiguousarray(c.own_plans)).to(dev), torch.from_numpy(c.own_has).to(dev)
    for prefilter in (1, -1):
        sol = hdsm.Solver(c.prm(prefilter_min_agents=prefilter), sc.N_ROB, sc.N_ROB)
        sol.set_plan_shift(c.shift)
        sol.set_own_plans_device(d_own, d_has)
        args = c.args(plans=c.decoy, has=c.decoy_has)
        compare(sol.replan(*args), want)                   # the host form goes through the same launch
        sol.reset_warm_start()
        compare(_device_replan(sol, c, args, dev), want)
        sol.set_own_plans_device(d_own, None)
        no_flag = c._per_instance(oracle, lambda a: sc.view_of(a, c.decoy, c.decoy_has, c.shift, c.own_plans, None))
        sol.reset_warm_start()
        compare(sol.replan(*args), no_flag)
        sol.set_own_plans_device(None, None)
        sol.reset_warm_start()
        compare(sol.replan(*args), c.want(oracle, "decoy"))
        sol.close()


@pytest.mark.parametrize("idx", range(len(sc.CASES)), ids=sc.IDS)
def test_shifted_reference_row_and_planes(hdsm, oracle, idx):
    """hdsm_reference_device (k_ref_pack, k_reference: the sphere path and, with a limit that is not monotone in the distance, the
    scan that reads the records directly) against orc_reference per instance on materialised records, without and with the own-plan
    override; hdsm_reference through the same launches; hdsm_tasc_planes against the oracle's planes."""
    import torch
    c = sc.case(idx)
    sn, N = c.sn, c.n_hor
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sol = hdsm.Solver(c.prm(), sc.N_ROB, sc.N_ROB)
    sol.set_plan_shift(c.shift)
    d_own, d_has = up(c.own_plans), up(c.own_has)
    d_id, d_path, d_np = up(sn["agent_id"]), up(c.path), up(c.n_path)
    for override in (False, True):
        plans, has = (c.decoy, c.decoy_has) if override else (sn["plans"], sn["has_plan"])
        if override:
            sol.set_own_plans_device(d_own, d_has)
        for monotone in (True, False):
            want = c.want_reference(oracle, monotone, override)
            full, ref, pv = (torch.zeros((sc.N_ROB, N + 1, 6), dtype=torch.float64, device=dev), torch.zeros((sc.N_ROB, N, 6), dtype=torch.float64, device=dev),
                             torch.zeros(sc.N_ROB, dtype=torch.float64, device=dev))
            sol.reference_device(c.ref_cfg(monotone), d_id, d_path, d_np, up(plans), up(has), full, ref, pv)
            torch.cuda.synchronize()
            host = sol.reference(c.ref_cfg(monotone), sn["agent_id"], c.path, c.n_path, plans, has)
            for got in ((full.cpu().numpy(), ref.cpu().numpy(), pv.cpu().numpy()), host):
                for g, w, name in zip(got, want, ("ref_full", "ref", "path_vel")):
                    err, scale = np.abs(g - w).max(), max(1.0, np.abs(w).max())
                    assert err < 1e-10 * scale, (override, monotone, name, err)
        planes = sol.tasc_planes(sn["agent_id"], sn["state"], plans, has)
        for a in range(sc.N_ROB):
            m, h = sc.view_of(a, plans, has, c.shift, c.own_plans if override else None, c.own_has if override else None)
            want_p, _ = oracle.tasc_planes(c.prm(), a, sn["state"][a], m, h)
            assert np.abs(planes[a] - want_p).max() < 1e-12, (override, a)
    sol.close()


def test_the_spheres_are_those_of_the_shifted_positions(hdsm, oracle):
    """tests/shift_cases.py, sphere_case: agent 8's record runs from 40 m away to beside agent 0. Unshifted, its sphere reaches every
    agent and every instance's sweeps load its N positions. Shifted by N it is one point beside agent 0: the answers equal the
    oracle's on the materialised record, agent 0's differs from the unshifted one, and the prefilter of agents 4..7 — metres from
    that point — now skips the neighbour: their sweeps load N fewer positions per pass than before. With `bounds` left unshifted the
    counts would not drop; with `pos` left unshifted the answers would be the unshifted ones. (The case the issue names, a culled
    unshifted sphere with an active shifted plane, cannot exist: tests/test_plan_shift.py.)"""
    prm, sn, shift = sc.sphere_case()
    prm.prefilter_min_agents = 1
    n, N = 9, prm.n_hor
    args = [sn[k] for k in ARG_KEYS]
    want = {k: np.concatenate([oracle.replan(prm, *[sn[q][a:a + 1] for q in ARG_KEYS[:7]], *sc.view_of(a, sn["plans"], sn["has_plan"], shift))[k]
                               for a in range(n)]) for k in ("traj", "ctrl", "status", "obj")}
    plain_want = oracle.replan(prm, *args)
    assert sc.moved(want, plain_want)[0] > 1e-3 and (want["status"][:8] != 2).all()       # (agent 8 itself, 40 m from its box, has no solution)
    sol = hdsm.Solver(prm, n, n)
    plain = sol.replan(*args)
    compare(plain, plain_want)
    st0, sw0 = sol.last_sweep_stats(n), sol.last_stats(n)["sweeps"]
    sol.reset_warm_start()
    sol.set_plan_shift(shift)
    got = sol.replan(*args)
    compare(got, want)
    st1, sw1 = sol.last_sweep_stats(n), sol.last_stats(n)["sweeps"]
    per0, per1 = st0["pairs"] / np.maximum(sw0, 1), st1["pairs"] / np.maximum(sw1, 1)
    print("positions loaded per sweep, unshifted:", per0.tolist(), "shifted:", per1.tolist())
    assert (sw0[4:8] > 0).all() and (sw1[4:8] > 0).all()
    assert (per1[4:8] <= per0[4:8] - N).all(), (per0.tolist(), per1.tolist())
    sol.close()


def test_argument_checks(hdsm):
    prm = sc.case(2).prm()
    sol = hdsm.Solver(prm, 16, 16)
    for bad in ([0, -1, 2], list(range(17))):
        with pytest.raises(hdsm.HdsmError) as e:
            sol.set_plan_shift(bad)
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    sol.set_plan_shift([1, 2, 3])                          # fewer than n_rob_max: the agents behind are unshifted
    L = hdsm.load()
    assert L.hdsm_set_own_plans_device(sol.h, None, np.zeros(1, np.uint8)) == hdsm.HDSM_ERR_BAD_ARG     # flags without plans
    sol.close()
