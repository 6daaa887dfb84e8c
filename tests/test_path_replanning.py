"""The path step (csrc/path_core.h; Agent::UpdatePath, agent_class.cpp:261-454, and GoalCallback, :2380-2388) on the CPU:
hdsm_local_path_host against an independent numpy restatement, the segments it returns, and goals changed in flight with the
oracle as the solver."""
import numpy as np
import pytest

import path_cases as pc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params


def _worlds():
    rng = np.random.default_rng(5)
    raw, origin = sc.forest_for_circle(48, seed=21)
    yield "forest", sc.inflate(raw), origin, (), (), 80, rng
    fwf, o2 = sc.forest_wall_forest(seed=3)
    yield "fwf", sc.inflate(fwf), o2, (), (), 70, rng
    for s in range(2):
        w, o3, sealed, blocks = pc.halo_world(np.random.default_rng(40 + s))
        yield "halo%d" % s, w, o3, sealed, blocks, 40, rng


def _host(world, cs):
    return lib.local_path_host(world, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"], res=pc.VS)


def test_local_path_host_equals_the_numpy_restatement():
    """>= 200 cases in the forest of cfg 3, the forest-wall-forest of cfg 5 and pillar worlds with a potential halo, sealed boxes
    and solid blocks: statuses, counts and every point bit for bit."""
    total, kinds = 0, set()
    for name, world, origin, sealed, blocks, n, rng in _worlds():
        cs = pc.make_cases(world, origin, n, rng, sealed=sealed, blocks=blocks)
        paths, n_path, status = _host(world, cs)
        for t in range(n):
            want_st, want = pc.plan(world, cs["off"][t], int(cs["ground_k"][t]), cs["origin"][t], cs["start"][t], cs["goal"][t])
            assert status[t] == want_st, (name, t, int(status[t]), want_st)
            assert n_path[t] == len(want), (name, t)
            if want:
                assert np.array_equal(paths[t, : n_path[t]], np.array(want)), (name, t, paths[t, : n_path[t]], want)
            kinds.add(int(status[t]))
            # goals outside the local grid are in the mix
            rel = cs["goal"][t] - cs["origin"][t]
            if not ((rel > 0) & (rel < np.array(pc.LDIM) * pc.VS)).all():
                kinds.add("outside")
        total += n
    assert total >= 200
    assert {0, 1, 2, "outside"} <= kinds, kinds


def test_returned_segments_are_free_and_free_space_is_the_straight_segment():
    for name, world, origin, sealed, blocks, n, rng in _worlds():
        cs = pc.make_cases(world, origin, n, rng, sealed=sealed, blocks=blocks)
        paths, n_path, status = _host(world, cs)
        checked = 0
        for t in np.nonzero(status == 0)[0]:
            occ = pc.occupancy(world, cs["off"][t], int(cs["ground_k"][t]))
            vox = lambda p: np.floor((p - cs["origin"][t]) / pc.VS).astype(int)
            s0 = vox(cs["start"][t])
            if occ[s0[2], s0[1], s0[0]]:
                continue  # (a start inside the inflation margin leaves it on its first segment)
            pts = paths[t, : n_path[t]]
            assert 2 <= len(pts) <= pc.PATH_PTS
            for a, b in zip(pts[:-1], pts[1:]):
                m = max(1, int(np.ceil(np.linalg.norm(b - a) / (pc.VS / 4))))
                for u in range(m + 1):
                    v = vox(a + (b - a) * (u / m))
                    assert not occ[v[2], v[1], v[0]], (name, t, a, b)
            checked += 1
        assert checked > n // 3, (name, checked)
    cs = pc.make_cases(np.zeros((20, 100, 100), np.int8), np.zeros(3), 20, np.random.default_rng(1))
    paths, n_path, status = lib.local_path_host(None, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
    assert (status == 0).all() and (n_path == 2).all()
    assert np.array_equal(paths[:, 0], cs["start"]) and np.array_equal(paths[:, 1], cs["goal"])


def _oracle_loop(oracle, prm, cfg, starts, goals, world=None):
    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"],
                             inp["A"], inp["b"], plans, has, n_threads=8)

    loop = swarm.SwarmLoop(prm, cfg, len(starts), solve=solve, starts=starts, goals=goals)
    if world is not None:
        loop.set_world(world[0], world[1], route=False)
    return loop


def _fly(loop, rounds, n):
    min_sep = 1e9
    for _ in range(rounds):
        loop.step()
        pos, dist, nfail = loop.shard.state()
        D = np.linalg.norm(pos[:, None] - pos[None], axis=2) + np.eye(n) * 1e9
        min_sep = min(min_sep, D.min())
        assert loop.shard.corridor_errors()[0] == 0
        assert loop.shard.path_errors()[0] == 0
    return min_sep


def test_new_goals_in_flight_with_the_oracle(oracle):
    """Eight agents swap places (100 rounds), then set_goals(starts) sends them back (100 rounds): everybody arrives within
    0.2 m, no collision, no failure."""
    prm = agile_params(10, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(8)
    loop = _oracle_loop(oracle, prm, cfg, starts, goals)
    sep = _fly(loop, 100, 8)
    assert loop.shard.state()[1].max() < 0.2
    loop.shard.set_goals(starts)
    sep = min(sep, _fly(loop, 100, 8))
    pos, dist, nfail = loop.shard.state()
    assert np.linalg.norm(pos - starts, axis=1).max() < 0.2
    assert nfail.sum() == 0 and sep > 2 * prm.drone_radius
    paths, n_path = loop.shard.get_paths()
    assert np.array_equal(paths[np.arange(8), n_path - 1], starts)  # (free space: [S, new goal])


def test_new_goals_in_a_forest_with_a_path_period(oracle):
    """The same flight through a small forest with set_path_period(1): a new path every round, no corridor or path error, every
    goal reached."""
    prm = agile_params(10, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(8, radius=8.0)
    raw, origin = sc.forest_for_circle(8, radius=8.0, density=0.06, seed=4)
    world = sc.inflate(raw)
    loop = _oracle_loop(oracle, prm, cfg, starts, goals, world=(world, origin))
    loop.shard.set_path_period(1)
    sep = _fly(loop, 100, 8)
    assert loop.shard.state()[1].max() < 0.2
    loop.shard.set_goals(starts)
    sep = min(sep, _fly(loop, 100, 8))
    pos, dist, nfail = loop.shard.state()
    assert dist.max() < 0.2 and np.linalg.norm(pos - starts, axis=1).max() < 0.2
    assert nfail.sum() == 0 and sep > 2 * prm.drone_radius
    paths, n_path = loop.shard.get_paths()
    assert (n_path >= 2).all()


def test_path_step_defaults_change_nothing():
    """No period, no goal change: the paths stay what hdsm_swarm_create / set_paths made them, and replan_paths in free space
    gives [S, goal]."""
    prm = agile_params(10, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(4)
    sh = swarm.SwarmShard(prm, cfg, 4, 0, starts, goals)
    sh.prepare(np.zeros((4, 11, 9)), np.zeros(4, np.uint8))
    paths, n_path = sh.get_paths()
    assert (n_path == 2).all() and np.array_equal(paths[:, 0], starts)
    sh.set_goals(goals)  # unchanged goals: nobody due
    assert sh.replan_paths() == 0 and sh.path_errors()[0] == 0
    paths, n_path = sh.get_paths()
    assert np.array_equal(paths[:, 1], goals)
    with pytest.raises(lib.HdsmError):
        sh.set_path_period(-1)
