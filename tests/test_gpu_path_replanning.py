"""The path step on the MI355X (k_path_batch / k_path, csrc/path_core.h): the device batch against the host form bit for bit, the
device-resident loop with a path period and with goals changed in flight against the host mirror, and the kernel's resources."""
import numpy as np
import pytest

import path_cases as pc
from flight_harness import _compare, device_loop, forest_pair, hdsm  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import _kernel_blocks, _kernel_descriptors
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import agile_params


@pytest.mark.gpu
def test_local_path_batch_equals_the_host_form(hdsm):  # noqa: F811
    """>= 1500 cases in the forest of cfg 3 and the forest-wall-forest of cfg 5 (and worlds with sealed boxes and solid blocks):
    hdsm_local_path_batch == hdsm_local_path_host, statuses, counts and points bit for bit."""
    rng = np.random.default_rng(17)
    raw, origin = sc.forest_for_circle(256, seed=13)
    fwf, o2 = sc.forest_wall_forest(seed=0)
    w3, o3, sealed, blocks = pc.halo_world(np.random.default_rng(3))
    total, ok = 0, 0
    for world, org, n, extra in ((sc.inflate(raw), origin, 800, {}), (sc.inflate(fwf), o2, 700, {}),
                                 (w3, o3, 120, dict(sealed=sealed, blocks=blocks))):
        cs = pc.make_cases(world, org, n, rng, **extra)
        args = (world, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
        pd, nd, sd = hdsm.local_path_batch(*args, res=pc.VS)
        ph, nh, sh = hdsm.local_path_host(*args, res=pc.VS)
        assert np.array_equal(sd, sh), np.nonzero(sd != sh)
        assert np.array_equal(nd, nh)
        assert np.array_equal(pd, ph), float(np.abs(pd - ph).max())
        total += n
        ok += int((sd == 0).sum())
    assert total >= 1500 and ok > total // 2
    # free space and a 12 m high grid (cfg 5's local grid: 66 x 66 x 40)
    cs = pc.make_cases(np.zeros((20, 100, 100), np.int8), np.zeros(3), 16, rng)
    a = (None, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
    assert all(np.array_equal(x, y) for x, y in zip(hdsm.local_path_batch(*a), hdsm.local_path_host(*a)))
    tall = (sc.inflate(fwf), (66, 66, 40), cs["off"] * 0 + [100, 20, 0], cs["ground_k"] * 0 + 20, np.array([[30.0, 6.0, -6.0]] * 16),
            np.array([[40.0, 16.0, 0.5]] * 16) + rng.uniform(-2, 2, (16, 3)), np.array([[60.0, 16.0, 1.0]] * 16) + rng.uniform(-3, 3, (16, 3)))
    bd, bh = hdsm.local_path_batch(*tall), hdsm.local_path_host(*tall)
    assert all(np.array_equal(x, y) for x, y in zip(bd, bh)) and (bd[2] == 0).any()


@pytest.mark.gpu
def test_device_loop_with_a_path_period_follows_the_host_mirror(hdsm):  # noqa: F811
    """set_path_period(1) in the forest (48 agents): k_path plans every agent every round, the host mirror with the same setting
    plans the same paths; 30 rounds agree to 1e-7 (the solver's staging order is not deterministic), paths bit for bit."""
    from multi_agent_pkgs_amd import swarm
    (_, host), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    for r in range(30):
        _compare(host, dsw, r)
    st = dsw.path_stats()
    assert st["planned"] == 30 * 48 and st["launches"] == 30
    dsw.download(states=True)
    pd, nd = dev_loop.shard.get_paths()
    ph, nh = host.shard.get_paths()
    assert np.array_equal(nd, nh) and np.abs(pd - ph).max() < 1e-7
    assert (dev_loop.shard.path_errors()[1] == host.shard.path_errors()[1]).all()
    dsw.close()


@pytest.mark.parametrize("scene", ["circle", "forest"])
@pytest.mark.gpu
def test_new_goals_in_flight_on_the_device(hdsm, scene):  # noqa: F811
    """set_goals in mid-flight: DeviceSwarm and the host mirror apply it the same way (10 rounds compared); then the device swarm
    flies on and reaches the new goals."""
    from multi_agent_pkgs_amd import swarm
    n_rob = 16
    prm = agile_params(10, max_rows_static=18)

    def make():  # (in the forest a path ends at the local grid's intermediate goal: it is planned again every round)
        sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
        if scene == "forest":
            raw, origin = sc.forest_for_circle(n_rob, seed=6)
            world = sc.inflate(raw)
            # (every new goal in a free voxel: a path to an occupied goal voxel ends at the nearest free voxel's centre)
            v = np.floor((sc.circle_scenario(n_rob)[0] - origin) / 0.3).astype(int)
            assert (world[v[:, 2], v[:, 1], v[:, 0]] < 100).all()
            assert loop.set_world(world, origin) == 0
            loop.pmax = 49
            loop.shard.set_path_period(1)
        return sol, loop

    (_, host), (sol_d, dev_loop) = make(), make()
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    starts, _ = sc.circle_scenario(n_rob)
    for r in range(20):
        _compare(host, dsw, r)
    host.shard.set_goals(starts)
    dsw.set_goals(starts)
    for r in range(20, 30):
        _compare(host, dsw, r)
    st = dsw.path_stats()
    if scene == "circle":
        assert st["planned"] == n_rob and st["launches"] == 1 and st["failed"] == 0
    else:
        assert st["planned"] == 30 * n_rob and st["launches"] == 30
    for r in range(30, 400):
        dsw.round()
    dsw.download(states=True)
    pos, dist, nfail = dev_loop.shard.state()
    assert np.linalg.norm(pos - starts, axis=1).max() < 0.2 and dist.max() < 0.2
    dsw.close()


@pytest.mark.gpu
def test_path_step_timing_is_reported(hdsm):  # noqa: F811
    from multi_agent_pkgs_amd import swarm
    (_, _), (sol_d, dev_loop) = forest_pair(hdsm, 64, 1)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    dsw.set_phase_timing(True)
    dsw.round()
    assert dsw.last_path_ms() > 0 and dsw.phase_ms()["k_corridor"] > 0
    dsw.close()


def test_k_path_has_no_scratch_and_fits_two_workgroups_per_cu(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    desc = _kernel_blocks(tmp_path / "a")
    assert sum(v.get("private_segment_fixed_size", 0) for k, v in _kernel_descriptors(tmp_path / "b").items() if "k_path" in k) == 0
    ks = {k: v for k, v in desc.items() if "k_path" in k}
    assert any("6k_path" in k for k in ks) and any("k_path_batch" in k for k in ks), sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert 0 < v["group_segment_fixed_size"] <= 80 * 1024, (k, v)
