"""GPU tests that FLY BASELINE.json's configurations 2, 3, 4 and 5 in closed loop on the device and check, at selected
rounds, size-independent properties on EVERY instance plus parity with the CPU oracle on a random subset:

  cfg 2   64 agents, circular exchange with the SHIPPED geometry (R = 22 m around (18, 15),
          multi_agent_planner_circle.launch.py:25-44), empty world, H = 10; every instance of the checked rounds against the oracle
  cfg 3   256 agents, circular exchange (R = 256 / 2 pi) through a pillar forest, corridors from the voxel decomposition
          (both GetPolyOcta3D and, where a seed is pinched, GetPolyOcta3DNew), H = 10
  cfg 4   1024 agents, circular exchange (R = 1024 / 2 pi), empty world, H = 10, flown THROUGH the rounds in which the
          contracting ring reaches the 0.5 m separation limit (rounds 165-185: hundreds of infeasible instances)
  cfg 5   4096 agents, y-z lattice through forest + wall + forest, H = 15, a few rounds

Properties (all instances with a solution): trajectory = literal rollout of the controls; input / velocity / acceleration
boxes and v_N = a_N = 0; every separating plane of every step holds at p_i and p_{i+1}; every segment lies in a polyhedron
flagged in poly_used; obj is the literal objective. Instances without a solution leave the outputs untouched (checked
through the host mirror's fallback: the published plan is the shifted previous one)."""
import numpy as np
import pytest

from flight_harness import device_loop, hdsm  # noqa: F401  (the module's fixture and loop builder)
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import agile_params

pytestmark = pytest.mark.gpu

TRAJ_TOL = 1e-7
OBJ_RTOL = 1e-6


def _check_round(sol, oracle, prm, rec, out, n_parity, rng, plane_chunk=32, traj_tol=TRAJ_TOL):
    """Properties on every solved instance of one recorded round + oracle parity on a random subset."""
    N, P = prm.n_hor, prm.poly_hor
    n = rec["state"].shape[0]
    status = out["status"]
    ok = np.where(status != 2)[0]
    traj, ctrl = out["traj"], out["ctrl"]
    # dynamics, boxes, objective
    for a in ok:
        assert np.abs(oracle.rollout(prm, rec["state"][a], ctrl[a]) - traj[a]).max() < 1e-9
        assert abs(oracle.objective(prm, traj[a], ctrl[a], rec["ref"][a]) - out["obj"][a]) < 1e-7 * max(1.0, abs(out["obj"][a]))
    assert np.abs(ctrl[ok]).max() <= 60 + 1e-8
    assert np.abs(traj[ok][:, 1:N, 3:6]).max() <= 20 + 1e-8 and np.abs(traj[ok][:, 1:N, 6:9]).max() <= 15 + 1e-8
    assert np.abs(traj[ok][:, N, 3:9]).max() < 1e-8
    # separating planes (device plane generator, itself checked against the literal chain in test_gpu_parity.py)
    for c0 in range(0, len(ok), plane_chunk):
        ids = ok[c0:c0 + plane_chunk]
        planes = sol.tasc_planes(rec["agent_id"][ids], rec["state"][ids], rec["plans"], rec["has_plan"])  # [m][N][n_rob][4]
        for e in (0, 1):
            pts = traj[ids][:, e:N + e, :3]                                                    # p_{i+e}
            viol = np.einsum("minc,mic->min", planes[..., :3], pts) - planes[..., 3]
            lim = np.full((1, N, 1), 1e-7)
            pinned = 0 if prm.rk4 else 2           # p_0 .. p_pinned do not depend on the inputs: rows there are constants judged
            for i in range(N):                     # with feas_tol_fixed
                if i + e <= pinned:
                    lim[0, i, 0] = 1e-6
            assert (viol < lim).all(), (ids[np.argmax(viol.max(axis=(1, 2)))], float(viol.max()))
    # containment in a polyhedron flagged used
    A, b, nr = rec["A"], rec["b"], rec["n_rows"]
    for a in ok:
        for i in range(N):
            inside = False
            for j in range(min(P, int(rec["n_poly"][a]))):
                if not out["used"][a, j]:
                    continue
                r = int(nr[a, j])
                v0 = (A[a, j, :r] @ traj[a, i, :3] - b[a, j, :r]).max()
                v1 = (A[a, j, :r] @ traj[a, i + 1, :3] - b[a, j, :r]).max()
                pinned = 0 if prm.rk4 else 2
                if v0 < (1e-6 if i <= pinned else 1e-7) and v1 < (1e-6 if i + 1 <= pinned else 1e-7):
                    inside = True
                    break
            assert inside, (a, i)
    # oracle parity on a random subset (instances the device stopped on a budget are checked by _check_limit_instances)
    sub = rng.choice(n, min(n_parity, n), replace=False)
    sub = sub[status[sub] != 1]
    o = _oracle_proved(oracle, prm, rec, sub)
    sub, o = sub[o["status"] != 1], {k: v[o["status"] != 1] for k, v in o.items()}   # (no verdict without a proof)
    assert (status[sub] == o["status"]).all(), (status[sub].tolist(), o["status"].tolist())
    good = o["status"] != 2
    if good.any():
        assert np.abs(traj[sub] - o["traj"])[good].max() < traj_tol
        rel = np.abs(out["obj"][sub] - o["obj"])[good] / np.maximum(1.0, np.abs(o["obj"][good]))
        assert rel.max() < OBJ_RTOL
    return len(ok), int((status == 2).sum())


def _oracle_proved(oracle, prm, rec, sub, hint=None, threads=0, nodes=200000, iters=30000000):
    """The oracle on instances `sub` of a recorded round, with a PROOF wherever the budgets allow one. H <= 10: the step-ordered
    search first (bounded), then — where that ran into its budget — the oracle's other search order (most infeasible step
    first), which finishes the trees the enumeration in step order cannot; H > 10: the second order directly. An oracle
    answer with status LIMIT (budget exhausted in both orders) is returned as such: the callers never compare against it."""
    keys = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")
    import os
    threads = threads or min(64, os.cpu_count() or 8)
    if prm.n_hor <= 10:
        bounded = prm.copy()
        bounded.max_nodes, bounded.max_qp_iters = 100000, 1000000
        o = oracle.replan(bounded, *[rec[k][sub] for k in keys], rec["plans"], rec["has_plan"], n_threads=threads)
        again = np.where(o["status"] == 1)[0]
    else:
        o, again = None, np.arange(len(sub))
    if len(again):
        big = prm.copy()
        big.max_nodes, big.max_qp_iters = nodes, iters
        o2 = oracle.replan(big, *[rec[k][sub[again]] for k in keys], rec["plans"], rec["has_plan"], n_threads=threads, search=1,
                           obj_hint=None if hint is None else hint[again])
        if o is None:
            return o2
        for k in ("traj", "ctrl", "used", "status", "obj", "nodes"):
            o[k][again] = o2[k]
    return o


def _check_limit_instances(sol, oracle, prm, rec, out, max_check=3):
    """Instances the device ended on a work budget (status LIMIT: an incumbent without a proof). Their incumbents have passed
    the property checks of _check_round like every other solution (feasible in every respect); here the oracle looks for the
    true optimum of up to `max_check` of them (hinted with the incumbent's objective, bounded budgets) and, where it gets a
    proof, the incumbent's objective must not be BELOW the optimum. Returns [(instance, flags, relative gap or None)]."""
    lim = np.where(out["status"] == 1)[0][:max_check]
    if len(lim) == 0:
        return []
    flags = sol.last_sweep_stats(len(out["status"]))["flags"][lim]
    o = _oracle_proved(oracle, prm, rec, lim, hint=out["obj"][lim] * (1 + 1e-9), threads=16, nodes=20000, iters=4000000)
    res = []
    for t, a in enumerate(lim):
        gap = None
        if o["status"][t] == 0:                                    # proven optimum (the hint only prunes: see orc_replan_ex)
            gap = float((out["obj"][a] - o["obj"][t]) / max(1.0, abs(o["obj"][t])))
            assert gap > -1e-7, (int(a), gap)                       # nothing can beat the optimum
        assert o["status"][t] != 2, int(a)                          # a feasible incumbent exists, so something must be found below the cut
        res.append((int(a), int(flags[t]), gap if o["status"][t] == 0 else "oracle budget exhausted"))
    return res


def test_config_2_64_agents_circle_shipped_geometry(hdsm, oracle):  # noqa: F811
    """BASELINE configs[1]: 64 agents, circular exchange, empty environment, H = 10 — the geometry of the reference's own
    launch file (R = 22 m, centre (18, 15), z = 1.5: chord 2.16 m), flown until the swarm has crossed; EVERY instance of
    every tenth round is compared with the oracle."""
    from multi_agent_pkgs_amd import swarm
    n_rob, N = 64, 10
    prm = agile_params(N, max_rows_static=18)
    starts, goals = sc.circle_scenario(n_rob, radius=22.0, cx=18.0, cy=15.0, z=1.5)
    assert np.allclose(starts[0], [40.0, 15.0, 1.5]) and np.allclose(goals[0], [-4.0, 15.0, 1.5])   # SURVEY 8d known answers
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob, starts=starts, goals=goals)
    rng = np.random.default_rng(2)
    solved = failed = multi = 0
    dmin = 1e9
    for r in range(180):
        rec = []
        out = loop.step(record=rec)
        pos, dist, _ = loop.shard.state()
        d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=2) + np.eye(n_rob) * 9
        dmin = min(dmin, float(d.min()))
        multi += int((out["used"].sum(axis=1) > 1).sum())
        if r % 10 == 9 or r in (64, 67, 73, 76):                    # + some rounds of the crossing
            # (EVERY instance of 13 rounds is compared: 1e-6 on the trajectories — the two exact solvers stop on different
            # active sets where the optimum is flat; the sampled checks of the other flights keep 1e-7, BASELINE asks for 1e-4)
            n_ok, n_bad = _check_round(sol, oracle, prm, rec[0], out, n_rob, rng, traj_tol=1e-6)
            assert _check_limit_instances(sol, oracle, prm, rec[0], out) == []
            solved += n_ok
            failed += n_bad
    assert solved > 20 * n_rob * 0.8 and dmin > 0.45                # nobody closer than the drone diameter (0.5 m) - tolerance
    assert multi > 100                                              # trajectories really span several corridor boxes (MIQP)
    assert dist.mean() < 0.4 * 44.0, float(dist.mean())             # the swarm got through the crossing
    print("cfg2: instance-solves checked against the oracle", solved, "without solution", failed, "closest approach", dmin,
          "distance to goal mean / max", float(dist.mean()), float(dist.max()))


def _pillar_hits(pos, raw, origin, vox=0.3):
    """Number of agent centres inside an (un-inflated) obstacle voxel. The corridor polyhedra are built on the INFLATED grid
    (0.3 m margin, drone radius 0.25 m), but like the reference's they are not exact: a chamfer plane may cut the corner of
    an inflated voxel, and a seed taken by an agent that sits in such a corner grows a polyhedron inside the margin
    (GetPolyOcta3D never tests the seed voxel, convex_decomp.cpp:49-52). In a gridlocked forest a few agents end up against a
    pillar this way; the tests bound how often."""
    v = np.floor((pos - origin) / vox).astype(int)
    inside = ((v >= 0) & (v < np.array(raw.shape[::-1]))).all(axis=1)
    v = v[inside]
    return int((raw[v[:, 2], v[:, 1], v[:, 0]] >= 100).sum())


def test_config_3_256_agents_through_a_forest(hdsm, oracle):  # noqa: F811
    """BASELINE configs[2]: 256 agents, forest environment, corridors by voxel decomposition (<= 4 polyhedra), H = 10."""
    from multi_agent_pkgs_amd import swarm
    n_rob, N = 256, 10
    prm = agile_params(N, max_rows_static=18)
    raw, origin = sc.forest_for_circle(n_rob, seed=13)
    occ = sc.inflate(raw)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
    assert loop.set_world(occ, origin) == 0                       # every agent has a route
    rng = np.random.default_rng(3)
    checked, rows_max, chamfered, hits = 0, 0, 0, 0
    for r in range(130):
        rec = []
        out = loop.step(record=rec)
        assert loop.shard.corridor_errors()[0] == 0
        rows_max = max(rows_max, int(rec[0]["n_rows"].max()))
        chamfered += int((rec[0]["n_rows"] > 6).any(axis=1).sum())
        pos, dist, _ = loop.shard.state()
        hits += _pillar_hits(pos, raw, origin)
        if r in (5, 40, 80, 110, 125):
            n_ok, n_bad = _check_round(sol, oracle, prm, rec[0], out, 64, rng)   # 64 of 256 instances per checked round against the oracle
            checked += n_ok
            assert n_ok > n_rob // 2
    assert rows_max > 6 and rows_max <= 18 and chamfered > 100    # the forest really shapes the corridors
    assert hits <= 0.001 * 130 * n_rob, hits                      # agent centres in an obstacle voxel: < 0.1 % of agent-rounds
    assert dist.mean() < 0.6 * 2 * n_rob / (2 * np.pi)            # the swarm made progress through the forest
    print("cfg3: instances checked", checked, "max static rows", rows_max, "agent-rounds inside an obstacle voxel", hits)


def test_config_4_1024_agents_circle_through_the_squeeze(hdsm, oracle):  # noqa: F811
    """BASELINE configs[3] on one GPU: 1024 agents, circular exchange, H = 10, through the rounds in which the contracting
    ring reaches the separation limit (the hard rounds of the flight: root relaxations become infeasible by the hundred)."""
    from multi_agent_pkgs_amd import swarm
    n_rob, N = 1024, 10
    prm = agile_params(N, max_rows_static=18)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
    rng = np.random.default_rng(4)
    bad_total, prev_plans = 0, None
    for r in range(186):
        rec = []
        out = loop.step(record=rec)
        if r in (100, 166, 170, 174, 180, 185):
            n_ok, n_bad = _check_round(sol, oracle, prm, rec[0], out, 24, rng)
            bad_total += n_bad
            # instances without a solution: the published plan is the previous one shifted by a step (AC:1000-1019)
            bad = np.where(out["status"] == 2)[0]
            if prev_plans is not None and len(bad):
                assert np.array_equal(loop.plans_all[bad][:, :N], prev_plans[bad][:, 1:])
                assert np.array_equal(loop.plans_all[bad][:, N], prev_plans[bad][:, N])
        prev_plans = loop.plans_all.copy()
    assert bad_total > 100                                          # the squeeze really is in the checked rounds
    pos, _, _ = loop.shard.state()
    d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=2) + np.eye(n_rob) * 9
    assert d.min() > 0.45                                           # nobody closer than the drone diameter (0.5 m) - tolerance


def test_config_5_4096_agents_forest_wall_forest(hdsm, oracle):  # noqa: F811
    """BASELINE configs[4] on one GPU: 4096 agents (64 x 64 lattice, 2.01 m pitch), forest + wall + forest, H = 15."""
    from multi_agent_pkgs_amd import swarm
    n_y = n_z = 64
    n_rob, N = n_y * n_z, 15
    prm = agile_params(N, max_rows_static=18)
    tiles_y = int(np.ceil((5 + 2.01 * n_y + 5) / 30))
    tiles_z = int(np.ceil((6 + 2.01 * n_z + 3) / 15))
    raw, origin = sc.forest_wall_forest(tiles_y, tiles_z, seed=0)
    occ = sc.inflate(raw)
    starts, goals = sc.lattice_scenario(n_y, n_z)
    cfg = swarm.default_swarm_config()
    cfg.grid_range[2], cfg.grid_z_min = 12.0, -6.0                 # voxel_grid_range of multi_agent_planner_long.launch.py:29
    sol, loop = device_loop(hdsm, prm, cfg, n_rob, starts=starts, goals=goals)
    assert loop.set_world(occ, origin) == 0
    rng = np.random.default_rng(5)
    rows_max, limited = 0, []
    for r in range(16):
        rec = []
        out = loop.step(record=rec)
        assert loop.shard.corridor_errors()[0] == 0
        rows_max = max(rows_max, int(rec[0]["n_rows"].max()))
        if r in (3, 15):
            n_ok, n_bad = _check_round(sol, oracle, prm, rec[0], out, 64, rng, plane_chunk=8)   # 64 random instances per checked round against the oracle
            assert n_ok > 0.9 * n_rob
        # instances that ended on the node budget: incumbent vs the proven optimum (a few per flight: the proofs are expensive)
        if (out["status"] == 1).any() and len(limited) < 8:
            limited += _check_limit_instances(sol, oracle, prm, rec[0], out, max_check=8 - len(limited))
    pos, _, _ = loop.shard.state()
    assert _pillar_hits(pos, raw, origin) == 0
    assert pos[:, 0].mean() > 3.0 and rows_max > 6                 # moving into the first forest on shaped corridors
    print("cfg5: instances that ended on a budget (instance, flags, relative gap to the proven optimum):", limited)


def test_voxel_decomposition_on_the_device_matches_the_host_bit_for_bit(hdsm):  # noqa: F811
    """Row f2 on the device (hdsm_poly_octa3d_batch, one thread per seed) against the host functions hdsm_poly_octa3d /
    hdsm_poly_octa3d_new on the same local grids: rows, row counts and the number of voxels taken must be IDENTICAL — for
    windows cut out of an inflated pillar forest and of forest + wall + forest (ground below, world border inside the
    window, both variants forced and the AC:1385-1395 choice), and for the 48 recorded cases of tests/golden."""
    import os
    from multi_agent_pkgs_amd import swarm
    import decomp_cases as dc
    rng = np.random.default_rng(11)
    ldim = dc.LDIM
    for wname, potential in (("forest", False), ("fwf", False), ("forest", True), ("fwf", True)):
        # (potential: values 1..99 around the obstacles — free for the growth, "not empty" for the shape-aware variant's chamfer test)
        occ2, origin = dc.world(wname, potential=potential, rng=rng)
        n = 1500 if not potential else 600
        off, seed, ground, variant, org = dc.cases(occ2, origin, n, rng)
        rows, n_rows, rc, cells = hdsm.poly_octa3d_batch(occ2, ldim, off, ground, seed, variant, org, n_it=42, res=0.3, max_rows=32)
        # the cooperative form (one wavefront per seed, workspace in LDS: what the device loop's corridor kernel runs) gives the
        # same rows, row counts, return codes and voxel counts, bit for bit
        w_rows, w_n, w_rc, w_cells = hdsm.poly_octa3d_batch(occ2, ldim, off, ground, seed, variant, org, n_it=42, res=0.3, max_rows=32, wave=True)
        assert np.array_equal(w_n, n_rows) and np.array_equal(w_rc, rc) and np.array_equal(w_cells, cells), wname
        valid = np.arange(32)[None, :] < n_rows[:, None]  # (rows beyond n_rows are not written)
        assert np.array_equal(w_rows[valid], rows[valid]), wname
        aware_cnt = chamfered = 0
        for t in range(n):
            want, voxels, v = dc.host_answer(occ2, off[t], seed[t], ground[t], variant[t], org[t])
            assert rc[t] == 0 and n_rows[t] == len(want), (wname, t)
            assert np.array_equal(rows[t, : n_rows[t]], want), (wname, t, rows[t, : n_rows[t]], want)
            assert cells[t] == voxels, (wname, t)
            aware_cnt += v
            chamfered += len(want) > 6
        assert aware_cnt > 20 and chamfered > n // 15, (aware_cnt, chamfered)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corridor_cases.npz"))
    for k in range(z["grids"].shape[0]):
        for v, key in ((0, "octa3d"), (1, "octa3d_new")):
            want = z["rows_" + key][k]
            want = want[~np.isnan(want[:, 0])]
            rows, n_rows, rc, cells = hdsm.poly_octa3d_batch(z["grids"][k], ldim, np.zeros((1, 3), np.int32), np.zeros(1, np.int32),
                                                             z["seeds"][k][None], np.array([v], np.int32), z["origin"][None],
                                                             n_it=int(z["n_it"][k]), res=float(z["res"]), max_rows=32)
            assert rc[0] == 0 and n_rows[0] == len(want) and np.array_equal(rows[0, : n_rows[0]], want), (k, key)
            assert cells[0] == int(z["cells_" + key][k])


@pytest.mark.parametrize("scene", ["circle", "forest"])
def test_device_resident_loop_follows_the_host_mirror(hdsm, scene):  # noqa: F811
    """hdsm_dswarm_round (corridor -> reference -> replan -> commit -> publish, all on the device, one stream) against the
    host-mirror loop that drives the same device kernels for the reference and the solve: same published plans round after
    round. The per-agent code is one source (csrc/swarm_core.h); the solver's staging order is not deterministic (atomics),
    so agreement is to 1e-7 over the first rounds, not bitwise. In the forest the corridors come from the device voxel
    decomposition (row f2) on a window of the world grid. (30 rounds: in round 36 of this forest flight agent 37 stands where
    1e-12 of noise in its position decides which voxel seeds its corridor — two handles then fly different, equally valid
    flights, scripts/gpu_debug_mirror.py.)"""
    from multi_agent_pkgs_amd import swarm
    n_rob, N, rounds = 48, 10, 30
    prm = agile_params(N, max_rows_static=18)

    def make():
        sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
        if scene == "forest":
            raw, origin = sc.forest_for_circle(n_rob, seed=21)
            assert loop.set_world(sc.inflate(raw), origin) == 0
        return sol, loop

    sol_h, host = make()
    sol_d, dev_loop = make()
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    chamfered = 0
    for r in range(rounds):
        rec = []
        out = host.step(record=rec)
        dsw.round()
        plans, has, status, failed = dsw.download(states=False)
        assert (has == host.has_plan).all(), r
        assert (status == out["status"]).all(), (r, status.tolist(), out["status"].tolist())
        assert np.abs(plans - host.plans_all).max() < 1e-7, (r, float(np.abs(plans - host.plans_all).max()))
        chamfered += int((rec[0]["n_rows"] > 6).any())
    if scene == "forest":
        assert chamfered > 5
    # the states come back into a host mirror and every host diagnostic works on them
    dsw.download(states=True)
    pos_d, dist_d, nf_d = dev_loop.shard.state()
    pos_h, dist_h, nf_h = host.shard.state()
    assert np.abs(pos_d - pos_h).max() < 1e-7 and (nf_d == nf_h).all()
    # ... and the host mirror can continue the flight from them
    dev_loop.plans_all, dev_loop.has_plan = plans, has
    out_d, out_h = dev_loop.step(), host.step()
    assert (out_d["status"] == out_h["status"]).all() and np.abs(dev_loop.plans_all - host.plans_all).max() < 1e-6


@pytest.mark.parametrize("scene", ["forest", "fwf"])
def test_device_corridor_kernel_matches_the_reference_restatement(hdsm, oracle, scene):  # noqa: F811
    """Row f2 on the device: k_corridor (one wavefront per agent, rows of the kept polyhedra in registers, cooperative voxel
    decomposition out of LDS) against oracle/hdsm_oracle.c: orc_safe_corridor — GenerateSafeCorridor (agent_class.cpp:1236-1447)
    restated from the reference text — on every agent of >= 50 rounds of the device-resident loop, in the world of BASELINE
    cfg 3 (pillar forest around a circle) and of cfg 5 (forest + wall + forest, H = 15): polyhedra, rows and seeds bit for bit."""
    import corridor_oracle as co
    from multi_agent_pkgs_amd import swarm
    from oracle import pyoracle as orc
    rounds = 52
    cfg = swarm.default_swarm_config()
    if scene == "forest":
        n_rob, N = 64, 10
        prm = agile_params(N, max_rows_static=18)
        sol, loop = device_loop(hdsm, prm, cfg, n_rob)
        raw, origin = sc.forest_for_circle(n_rob, seed=13)
    else:
        n_y, N = 8, 15
        n_rob = n_y * n_y
        prm = agile_params(N, max_rows_static=18)
        starts, goals = sc.lattice_scenario(n_y, n_y)
        cfg.grid_range[2], cfg.grid_z_min = 12.0, -6.0
        sol, loop = device_loop(hdsm, prm, cfg, n_rob, starts=starts, goals=goals)
        raw, origin = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
    assert loop.set_world(sc.inflate(raw), origin) == 0
    dsw = swarm.DeviceSwarm(loop.shard, sol)
    made = carried = 0
    for r in range(rounds):
        dsw.download(states=True)
        pre, prm_s, cfg_s, world, worigin = co.export_agents(loop.shard)
        dsw.round()
        dsw.download(states=True)
        post = co.export_agents(loop.shard)[0]
        for a in range(n_rob):
            rc, want = co.oracle_corridor(orc.lib(), prm_s, cfg_s, world, worigin, pre[a])
            got = co.product_corridor(post[a])
            if rc != 0 or post[a].corridor_rc != 0:   # (a seed outside the local grid / a polyhedron beyond the row capacity: both stop)
                assert rc != 0 and post[a].corridor_rc != 0, (r, a, rc, post[a].corridor_rc)
                continue
            assert co.same_corridor(got, want), (scene, r, a, [g[0] for g in got], [w[0] for w in want])
            old = co.product_corridor(pre[a])
            carried += sum(1 for g in got if any(np.array_equal(g[3], h[3]) for h in old))
            made += len(got)
    assert made - carried > n_rob and carried > n_rob   # polyhedra were generated AND carried over
    # ... and a good part of the generated ones were NOT grown but formed from the polyhedron cache (hdsm_dswarm_cache_stats) — through
    # the same-grid rule and, mostly, through the interior rule (same world voxel asked for from another local grid at the same
    # height): the oracle above grows every polyhedron, so every cache hit of these rounds was compared with a grown one bit for bit
    cs = dsw.cache_stats()
    assert cs["cache_on"] and cs["asked"] >= made - carried, cs
    assert cs["hits_interior"] > 0 and cs["hits_same_grid"] + cs["hits_interior"] > cs["asked"] // 10, cs
    dsw.close()
