"""Neighbour groups on the MI355X (ABI 1.8): hdsm_set_groups in the solver, the plane generator and the reference kernel, the
grouped device loop against the grouped host mirror, copies of one swarm at identical coordinates, the per-group report.

The definition under test: every result for agent a is what the ungrouped code returns when has_plan is zeroed for every agent
outside a's group. So every test compares with the oracle, or with the handle after the partition was cleared, fed masked flags.
Tolerances: those of tests/test_gpu_parity.py."""
import numpy as np
import pytest

import problems
from flight_harness import circle_flight, device_loop, hdsm  # noqa: F401  (hdsm: the module's fixture)
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config
from parity_cases import ARG_KEYS, compare

pytestmark = pytest.mark.gpu

G16 = [0, 1, 3, 8, 16]
CASES = [(10, 16, dict(seed=4, spacing=1.0), G16),
         (10, 16, dict(seed=3, narrow=True, turn=True), G16),
         (6, 16, dict(seed=4, spacing=1.0), G16),
         (15, 24, dict(seed=115, turn=True, spacing=1.2), [0, 5, 6, 24]),          # the NV = 48 kernel
         (10, 64, dict(seed=7, spacing=1.5, turn=True), [0, 7, 8, 40, 64])]
# the launch forms tests/test_gpu_fuzz.py forces by environment: shared-CU kernels with the sphere list inside groups, the
# four-per-CU kernel, the split launch
FORMS = {"shared-cu-prefilter": dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_ORDER_MIN="1", HDSM_BOUNDS_MIN="1"),
         "quad": dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_QUAD_MIN="1"),
         "split": dict(HDSM_SPLIT="1", HDSM_SPLIT_BUDGET="2")}


def _masked(has, lo, hi):
    m = np.zeros_like(has)
    m[lo:hi] = has[lo:hi]
    return m


def _pairs(groups):
    return list(zip(groups[:-1], groups[1:]))


def _per_group(solve, sn, groups):
    """solve(args) once per group, on the group's instances with has_plan masked to the group; the outputs put together."""
    outs = []
    for lo, hi in _pairs(groups):
        args = [sn[k][lo:hi] if k not in ("plans", "has_plan") else sn[k] for k in ARG_KEYS]
        args[-1] = _masked(sn["has_plan"], lo, hi)
        outs.append(solve(args))
    return {k: np.concatenate([o[k] for o in outs]) for k in ("traj", "ctrl", "status", "obj")}


_snapshots = {}


def _case(oracle, idx):
    """(prm, snapshot, groups, the oracle's answer per group, the oracle's ungrouped answer): computed once per case."""
    if idx not in _snapshots:
        n_hor, n_rob, kw, groups = CASES[idx]
        prm = agile_params(n_hor, max_rows_static=18)
        sn = problems.swarm_snapshot(prm, n_rob, **kw)
        want = _per_group(lambda args: oracle.replan(prm, *args, n_threads=8), sn, groups)
        _snapshots[idx] = (prm, sn, groups, want)
    return _snapshots[idx]


def _differs(a, b):
    """instances whose answers differ: another status, or trajectories more than 1e-4 apart"""
    both = (a["status"] != 2) & (b["status"] != 2)
    moved = np.abs(a["traj"] - b["traj"]).reshape(len(both), -1).max(1) > 1e-4
    return int(((a["status"] != b["status"]) | (both & moved)).sum())


def _check_sweep_bound(sol, prm, n_inst, groups):
    """a sweep reads (neighbour, step) positions of its own group only: pairs <= sweeps * N * size(group)"""
    size = np.concatenate([np.full(hi - lo, hi - lo) for lo, hi in _pairs(groups)])
    pairs, sweeps = sol.last_sweep_stats(n_inst)["pairs"], sol.last_stats(n_inst)["sweeps"]
    assert (pairs <= sweeps * prm.n_hor * size).all(), (pairs.tolist(), sweeps.tolist())


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: f"h{CASES[i][0]}-n{CASES[i][1]}-seed{CASES[i][2]['seed']}")
def test_grouped_replan_matches_oracle_and_masked_calls(hdsm, oracle, idx):  # noqa: F811
    prm, sn, groups, want = _case(oracle, idx)
    n = sn["state"].shape[0]
    args = [sn[k] for k in ARG_KEYS]
    sol = hdsm.Solver(prm, n, n)
    plain = sol.replan(*args)
    sol.set_groups(groups)
    for rep in range(2):          # (the second call starts from the first one's working sets)
        g = sol.replan(*args)
        compare(g, want)
        _check_sweep_bound(sol, prm, n, groups)
    assert _differs(g, plain) >= 1            # a partition that is ignored cannot pass
    sol.set_groups(None)
    sol.reset_warm_start()
    compare(g, _per_group(lambda a: sol.replan(*a), sn, groups))   # the code path of before the partition, masked
    again = sol.replan(*args)
    assert (again["status"] == plain["status"]).all()
    sol.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("idx", [0, len(CASES) - 1], ids=["first", "last"])
def test_grouped_replan_in_every_launch_form(hdsm, oracle, monkeypatch, idx, form):  # noqa: F811
    prm, sn, groups, want = _case(oracle, idx)
    n = sn["state"].shape[0]
    for k_, v_ in FORMS[form].items():
        monkeypatch.setenv(k_, v_)
    sol = hdsm.Solver(prm, n, n)
    for k_ in FORMS[form]:
        monkeypatch.delenv(k_)
    sol.set_groups(groups)
    for rep in range(2):
        g = sol.replan(*[sn[k] for k in ARG_KEYS])
        compare(g, want)
        _check_sweep_bound(sol, prm, n, groups)
    if form == "shared-cu-prefilter":
        assert (sol.last_sweep_stats(n)["sphere_records"] > 0).any()      # the sphere list ran, inside the groups
    sol.close()


def test_set_groups_argument_checks(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sol = hdsm.Solver(prm, 16, 16)
    for bad in ([1, 3, 16], [0, 3, 3, 16], [0, 8, 3, 16], [0, 8, 17]):
        with pytest.raises(hdsm.HdsmError) as e:
            sol.set_groups(bad)
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    sol.set_groups([0, 8, 16])
    sn = problems.swarm_snapshot(prm, 12, seed=31)
    with pytest.raises(hdsm.HdsmError) as e:       # n_rob < n_total
        sol.replan(*[sn[k] for k in ARG_KEYS])
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    # n_rob > n_total: the ids behind the partition belong to no group and are nobody's neighbour
    sol.set_groups([0, 4, 10])
    planes = sol.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"])
    assert (planes[:, :, 10:] == 0).all() and (planes[10:] == 0).all() and (planes[:4, :, :4] != 0).any()
    g = sol.replan(*[sn[k] for k in ARG_KEYS])
    sol.set_groups(None)
    sol.reset_warm_start()
    compare(g, _per_group(lambda a: sol.replan(*a), sn, [0, 4, 10, 11, 12]))      # (an agent behind the partition: alone)
    sol.close()


def test_grouped_planes(hdsm, oracle):  # noqa: F811
    """hdsm_tasc_planes, 12 agents in [0,4,12]: rows inside the group equal the oracle's to 1e-12, rows outside are zeros."""
    prm = agile_params(10)
    groups = [0, 4, 12]
    sn = problems.swarm_snapshot(prm, 12, seed=31, spacing=0.8)
    sol = hdsm.Solver(prm, 12, 12)
    sol.set_groups(groups)
    planes = sol.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"])
    for lo, hi in _pairs(groups):
        for k in range(lo, hi):
            ref, valid = oracle.tasc_planes(prm, k, sn["state"][k], sn["plans"], sn["has_plan"])
            assert np.abs(planes[k][:, lo:hi] - ref[:, lo:hi]).max() < 1e-12
            assert (planes[k][:, :lo] == 0).all() and (planes[k][:, hi:] == 0).all()
            others = [j for j in range(lo, hi) if j != k]
            assert (np.abs(planes[k][:, others, :3]).max(axis=2) > 0).all()       # ... and the rows inside are there
    sol.close()


def _reference_inputs(sn):
    n = sn["state"].shape[0]
    path = np.zeros((n, 3, 3))
    path[:, 0] = sn["state"][:, :3]
    path[:, 1] = path[:, 0] + [6.0, 2.0, 0.0]
    path[:, 2] = path[:, 1] + [0.0, 30.0, 0.5]
    return path, np.full(n, 3, np.int32)


def test_grouped_reference_is_the_masked_reference(hdsm):  # noqa: F811
    """hdsm_reference on the 16-agent snapshot: path_vel and ref_full equal the per-group masked calls of a handle without a
    partition bit for bit (a minimum does not depend on the order); at least one path_vel differs from the ungrouped call."""
    prm = agile_params(10, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 16, seed=4, spacing=1.0)
    path, n_path = _reference_inputs(sn)
    rcfg = agile_ref_config()
    sol = hdsm.Solver(prm, 16, 16)
    full0, _, pv0 = sol.reference(rcfg, sn["agent_id"], path, n_path, sn["plans"], sn["has_plan"])
    sol.set_groups(G16)
    full, ref, pv = sol.reference(rcfg, sn["agent_id"], path, n_path, sn["plans"], sn["has_plan"])
    sol.set_groups(None)
    for lo, hi in _pairs(G16):
        f, r, p = sol.reference(rcfg, sn["agent_id"][lo:hi], path[lo:hi], n_path[lo:hi], sn["plans"], _masked(sn["has_plan"], lo, hi))
        assert p.tobytes() == pv[lo:hi].tobytes() and f.tobytes() == full[lo:hi].tobytes() and r.tobytes() == ref[lo:hi].tobytes()
    assert (pv != pv0).any() and pv[0] == rcfg.path_vel_max        # (a group of one meets nobody)
    # one group, and the partition cleared: the handle that never heard of groups
    sol.set_groups([0, 16])
    full1, _, pv1 = sol.reference(rcfg, sn["agent_id"], path, n_path, sn["plans"], sn["has_plan"])
    assert pv1.tobytes() == pv0.tobytes() and full1.tobytes() == full0.tobytes()
    sol.close()


def test_one_group_and_no_group_are_the_ungrouped_handle(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 16, seed=4, spacing=1.0)
    args = [sn[k] for k in ARG_KEYS]
    never = hdsm.Solver(prm, 16, 16)
    want, planes = never.replan(*args), never.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"])
    sol = hdsm.Solver(prm, 16, 16)
    for setting in ([0, 16], G16, None):
        sol.set_groups(setting)
        if setting is G16:
            continue
        sol.reset_warm_start()
        compare(sol.replan(*args), want)
        assert sol.tasc_planes(sn["agent_id"], sn["state"], sn["plans"], sn["has_plan"]).tobytes() == planes.tobytes()
    never.close(), sol.close()


# ---- the device loop ------------------------------------------------------------------------------------------------------------
FOREST_GROUPS = [0, 5, 6, 24]
ROUNDS = 6


def _grouped_audit_host(hdsm, plans, has, groups, prm, world, origin):  # noqa: F811
    """the host form of the audit, one group at a time through has_plan (the public entry point has no partition)"""
    return np.concatenate([hdsm.flight_audit_host(plans, _masked(has, lo, hi), step_plan=1, first=lo, n_local=hi - lo, drone_radius=prm.drone_radius,
                                                  drone_z_offset=prm.drone_z_offset, world=world, worigin=origin, voxel_size=0.3)
                           for lo, hi in _pairs(groups)])


@pytest.fixture(scope="module")
def forest_flight(hdsm):  # noqa: F811
    """24 agents in [0,5,6,24] through the small forest of the path tests, path period 1, audit on: 6 rounds of the grouped device
    loop next to the grouped host mirror. What each round left is kept for the tests below; the dswarm stays open for the report."""
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    n = FOREST_GROUPS[-1]
    raw, origin = sc.forest_for_circle(n, seed=21)
    world = sc.inflate(raw)

    def make():
        sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n)
        assert loop.set_world(world, origin) == 0
        loop.pmax = 49
        loop.shard.set_path_period(1)
        loop.shard.set_groups(FOREST_GROUPS)
        loop.shard.set_audit(True, 1.0)
        return sol, loop

    (sol_h, host), (sol_d, dev) = make(), make()
    sol_h.set_groups(FOREST_GROUPS)          # the mirror's rounds call the solver themselves
    dsw = swarm.DeviceSwarm(dev.shard, sol_d)
    before = None
    rounds = []
    for r in range(ROUNDS):
        out = host.step()
        dsw.round()
        plans, has, status, failed = dsw.download(states=False)
        rounds.append(dict(host_plans=host.plans_all.copy(), host_has=host.has_plan.copy(), host_status=out["status"].copy(), plans=plans, has=has,
                           status=status, audit=dsw.last_audit_round(), host_audit=_grouped_audit_host(hdsm, plans, has, FOREST_GROUPS, prm, world, origin)))
    yield dict(prm=prm, host=host, dev=dev, dsw=dsw, rounds=rounds, before=before)
    dsw.close(), sol_h.close(), sol_d.close()


def test_grouped_device_loop_follows_the_grouped_host_mirror(forest_flight):
    f = forest_flight
    for r, rd in enumerate(f["rounds"]):
        assert (rd["has"] == rd["host_has"]).all(), r
        assert (rd["status"] == rd["host_status"]).all(), (r, rd["status"].tolist(), rd["host_status"].tolist())
        assert np.abs(rd["plans"] - rd["host_plans"]).max() < 1e-7, (r, float(np.abs(rd["plans"] - rd["host_plans"]).max()))
        for lo, hi in _pairs(FOREST_GROUPS):
            p = rd["audit"]["partner"][lo:hi]
            assert (((p >= lo) & (p < hi)) | (p < 0)).all(), (r, lo, p.tolist())
        assert rd["audit"].tobytes() == rd["host_audit"].tobytes(), r
    last = f["rounds"][-1]["audit"]
    assert last["partner"][5] == -1 and (last["partner"][:5] >= 0).all() and (last["partner"][6:] >= 0).all()
    f["dsw"].download(states=True)
    assert (f["dev"].shard.corridor_errors()[1] == f["host"].shard.corridor_errors()[1]).all()
    assert (f["dev"].shard.path_errors()[1] == f["host"].shard.path_errors()[1]).all()


def _fold(rep, status, n_fail, dist_goal, groups):
    """the per-group report from the per-agent records: swarm.flight_summary per slice, the failures, the last statuses"""
    from multi_agent_pkgs_amd import lib, swarm
    out = np.zeros(len(groups) - 1, lib.GROUP_REPORT)
    for g, (lo, hi) in enumerate(_pairs(groups)):
        o = out[g]
        o["first"], o["count"], o["n_local"] = lo, hi - lo, hi - lo
        o["no_solution_last"], o["failed_total"], o["dist_goal_max"] = (status[lo:hi] == 2).sum(), n_fail[lo:hi].sum(), dist_goal[lo:hi].max()
        o["sep_agent"] = o["sep_partner"] = o["sep_round"] = -1
        if rep is None:
            continue
        s = swarm.flight_summary(rep[lo:hi], first_id=lo)
        for k in ("rounds", "positions", "close_rounds", "occupied", "unknown", "crossed", "pot_sum"):
            o[k] = s[k]
        o["speed_max"] = rep["speed_max"][lo:hi].max()
        o["sep2_min"] = np.finfo(np.float64).max
        if s["sigma_min_agent"] >= 0:
            a = s["sigma_min_agent"]
            o["sep2_min"], o["sep_agent"], o["sep_partner"] = rep["sep2_min"][a], a, s["sigma_min_partner"]
            o["sep_substep"], o["sep_round"] = s["sigma_min_substep"], s["sigma_min_round"]
    return out


def _same_records(got, want):
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), (name, got[name].tolist(), want[name].tolist())


def test_group_report_is_the_fold_of_the_agent_records(forest_flight):
    f = forest_flight
    dsw, shard = f["dsw"], f["dev"].shard
    got = dsw.group_report()
    _, _, status, _ = dsw.download(states=True)
    _, dist_goal, n_fail = shard.state()
    _same_records(got, _fold(dsw.flight_report(), status, n_fail, dist_goal, FOREST_GROUPS))
    assert got["rounds"].tolist() == [ROUNDS] * 3 and got["sep_agent"][1] == -1 and (got["sep_agent"][[0, 2]] >= 0).all()


def test_copies_of_one_swarm_fly_the_same_flight(hdsm):  # noqa: F811
    """Four copies of one 6-agent circle exchange at IDENTICAL coordinates as the groups [0,6,12,18,24], free space, 8 rounds:
    every group flies group 0's flight and the flight of a plain 6-agent dswarm (1e-7, statuses equal). Before the audit was
    ever on, the audit fields of the group report are zeros and -1. Without the partition the same 24 agents start coincident,
    four at every point. They are NOT stuck (measured: 0 of 24 instances without a solution in each of the 8 rounds — two agents
    at exactly the same position build no plane, AC:1100-1205 normalises a zero vector to the row 0 . p <= 0), but they fly
    another flight: a twin at distance 0 holds every path velocity at path_vel_min (AC:1769-1817), and the plans leave the grouped
    ones by 0.8 - 2.4 m from the second round on. The test states that difference."""
    prm = agile_params(10, max_rows_static=18)
    starts6, goals6 = sc.circle_scenario(6, radius=5.0)
    starts, goals, groups = sc.repeat_scenario(starts6, goals6, 4)
    assert groups.tolist() == [0, 6, 12, 18, 24]
    sol1, loop1, one = circle_flight(hdsm, prm, starts6, goals6)
    sol4, loop4, four = circle_flight(hdsm, prm, starts, goals, groups=groups)
    solu, loopu, ungrouped = circle_flight(hdsm, prm, starts, goals)
    unsolved = 0
    for r in range(8):
        one.round(), four.round(), ungrouped.round()
        p1, h1, s1, _ = one.download(states=False)
        p4, h4, s4, _ = four.download(states=False)
        for g in range(4):
            sl = slice(6 * g, 6 * g + 6)
            assert (s4[sl] == s4[:6]).all() and (s4[sl] == s1).all() and (h4[sl] == h1).all(), (r, g)
            assert np.abs(p4[sl] - p4[:6]).max() < 1e-7 and np.abs(p4[sl] - p1).max() < 1e-7, (r, g)
        assert (s4 != 2).all(), r
        pu, hu, su, _ = ungrouped.download(states=False)
        unsolved += int((su == 2).sum())
        print(f"round {r}: ungrouped instances without a solution {int((su == 2).sum())} of 24, |plans - grouped| {np.abs(pu - p4).max():.3e}")
    # the same 24 agents without the partition: four agents at every point, every one slowed down by its twins
    assert np.abs(pu - p4).max() > 1e-3 and unsolved == 0
    rep = four.group_report()
    _, _, status, _ = four.download(states=True)
    _, dist_goal, n_fail = loop4.shard.state()
    _same_records(rep, _fold(None, status, n_fail, dist_goal, groups))
    whole = one.group_report()           # no partition: one record for the whole swarm
    assert whole.shape == (1,) and whole["first"][0] == 0 and whole["count"][0] == 6 and whole["sep_partner"][0] == -1
    for x in (one, four, ungrouped, sol1, sol4, solu):
        x.close()
