"""The path step's clearance mode on the MI355X (k_dmp_batch / k_dmp, csrc/path_core.h 6a-7'): the device batch against the host form
bit for bit, the device-resident loop in clearance mode against the host mirror, and the timing hook."""
import numpy as np
import pytest

import dmp_cases as dc
import path_cases as pc
from flight_harness import _compare, forest_pair, hdsm  # noqa: F401  (hdsm: the module's fixture)


def _same(dev, host):
    (pd, nd, sd, cd, rd), (ph, nh, sh, ch, rh) = dev, host
    assert np.array_equal(sd, sh), (np.nonzero(sd != sh)[0][:8], sd[sd != sh][:8], sh[sd != sh][:8])
    assert np.array_equal(cd, ch), (np.nonzero(cd != ch)[0][:8], cd[cd != ch][:8], ch[cd != ch][:8])
    assert np.array_equal(rd, rh) and np.array_equal(nd, nh)
    assert np.array_equal(pd, ph), float(np.abs(pd - ph).max())


@pytest.mark.gpu
def test_local_path_dmp_batch_equals_the_host_form(hdsm):  # noqa: F811
    """>= 1500 cases in the pre-processed forest of cfg 3 and forest-wall-forest of cfg 5 and a halo world (sealed boxes, solid
    blocks), cfg 5's 66 x 66 x 40 local grid, free space, no tunnel and a narrow tunnel: hdsm_local_path_dmp_batch ==
    hdsm_local_path_dmp_host, status, cost, n_raw, counts and points bit for bit."""
    rng = np.random.default_rng(17)
    counts = {"forest": 800, "fwf": 700, "halo3": 120}
    total, ok = 0, 0
    kept = {}
    for name, world, org, sealed, blocks in dc.worlds(hdsm.map_preprocess, forest_seed=13, fwf_seed=0, halo_seeds=(3,)):
        n = counts[name]
        cs = pc.make_cases(world, org, n, rng, sealed=sealed, blocks=blocks)
        args = (world, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
        dev = hdsm.local_path_dmp_batch(*args, search_rad=dc.SEARCH_RAD, res=pc.VS)
        host = hdsm.local_path_dmp_host(*args, search_rad=dc.SEARCH_RAD, res=pc.VS)
        _same(dev, host)
        total += n
        ok += int((dev[2] == 0).sum())
        kept[name] = (world, cs)
        print(name, "statuses", np.bincount(dev[2], minlength=5).tolist(), "cost max", int(dev[3].max()), "n_raw max", int(dev[4].max()))
    assert total >= 1500 and ok > total // 2
    # no tunnel (every free voxel of the grid) and a one-voxel tunnel
    for name, rad in (("forest", -1.0), ("fwf", -1.0), ("halo3", 0.3)):
        world, cs = kept[name]
        a = (world, pc.LDIM, cs["off"][:48], cs["ground_k"][:48], cs["origin"][:48], cs["start"][:48], cs["goal"][:48])
        dev = hdsm.local_path_dmp_batch(*a, search_rad=rad, res=pc.VS)
        _same(dev, hdsm.local_path_dmp_host(*a, search_rad=rad, res=pc.VS))
        assert (dev[2] == 0).any()
    # free space and a 12 m high grid (cfg 5's local grid: 66 x 66 x 40)
    cs = pc.make_cases(np.zeros((20, 100, 100), np.int8), np.zeros(3), 16, rng)
    a = (None, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
    dev = hdsm.local_path_dmp_batch(*a)
    _same(dev, hdsm.local_path_dmp_host(*a))
    assert (dev[2] == 0).all() and (dev[1] == 2).all() and (dev[3] == 0).all()
    fwf = kept["fwf"][0]
    tall = (fwf, (66, 66, 40), cs["off"] * 0 + [100, 20, 0], cs["ground_k"] * 0 + 20, np.array([[30.0, 6.0, -6.0]] * 16),
            np.array([[40.0, 16.0, 0.5]] * 16) + rng.uniform(-2, 2, (16, 3)), np.array([[60.0, 16.0, 1.0]] * 16) + rng.uniform(-3, 3, (16, 3)))
    dev = hdsm.local_path_dmp_batch(*tall)
    _same(dev, hdsm.local_path_dmp_host(*tall))
    assert (dev[2] == 0).any()


@pytest.mark.gpu
def test_device_loop_in_clearance_mode_follows_the_host_mirror(hdsm):  # noqa: F811
    """48 agents in the pre-processed forest, clearance 1.8, path period 1: k_dmp plans every agent every round, the host mirror
    with the same setting plans the same paths; 30 rounds agree to 1e-7, statuses, paths and path errors equal."""
    from multi_agent_pkgs_amd import swarm
    (_, host), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1, lambda raw: dc.preprocessed(raw, hdsm.map_preprocess), clearance=1.8)
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
    assert (nh > 2).any()  # (the mode is on: a plain path across the forest's edge would do with fewer points)
    dsw.close()


@pytest.mark.gpu
def test_clearance_path_step_timing_is_reported(hdsm):  # noqa: F811
    from multi_agent_pkgs_amd import swarm
    (_, _), (sol_d, dev_loop) = forest_pair(hdsm, 64, 1, lambda raw: dc.preprocessed(raw, hdsm.map_preprocess), clearance=1.8)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    dsw.set_phase_timing(True)
    dsw.round()
    assert dsw.last_path_ms() > 0 and dsw.phase_ms()["k_corridor"] > 0
    dsw.close()
