"""Map updates in flight on the MI355X: the region form of the map pre-processing against the full-grid form bit for bit, the
device-resident loop against the host mirror across edits of the world (processed and raw), the selectivity of the cache
invalidation, a takeover after edits, the new kernels' resources, and "off means off"."""
import numpy as np
import pytest

import world_cases as wu
from flight_harness import PLAN_TOL, _compare, device_loop, forest_pair, hdsm  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import LIB, _kernel_descriptors
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import default_map_config

LOOK = (42 + 5) // 6 + 2 + 1   # wave_map_radius(n_it_decomp = 42) and the voxel of margin: what an invalidation looks at round a seed
MAP_CFG = dict(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4)


def _boxes(dim):
    """(lo, bdim) in (x, y, z): one voxel, 3 wide, on each face, in two corners, ending at nx - 1, spanning the grid in x, the whole grid."""
    nx, ny, nz = dim
    mid = [nx // 2, ny // 2, nz // 2]
    out = [(mid, [1, 1, 1]), ([mid[0] - 1, mid[1], mid[2]], [3, 1, 1]), ([nx - 3, mid[1], mid[2] - 1], [3, 2, 2]), ([0, mid[1], mid[2]], [nx, 1, 1]),
           ([0, 0, 0], [nx, ny, nz]), ([0, 0, 0], [2, 2, 2]), ([nx - 2, ny - 1, nz - 2], [2, 1, 2])]
    for ax in range(3):
        for side in (0, 1):
            bd = [2, 3, 2]
            lo = [mid[0] - 1, mid[1] - 1, mid[2] - 1]
            lo[ax] = 0 if side == 0 else dim[ax] - bd[ax]
            out.append((lo, bd))
    return out


def _fill(raw, lo, bd, value):
    out = raw.copy()
    out[lo[2]:lo[2] + bd[2], lo[1]:lo[1] + bd[1], lo[0]:lo[0] + bd[0]] = value
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("setting", wu.SETTINGS)
def test_region_preprocessing_equals_the_full_grid_form(hdsm, setting):  # noqa: F811
    """hdsm_map_preprocess_region from the processed old grid == hdsm_map_preprocess of the edited raw grid, the WHOLE array bit for
    bit (a write outside W shows too). Grids 40 x 37 x 23 and 13 x 9 x 6; every box of _boxes redrawn at random and — the boxes on
    the faces and in the corners — filled with occupied, free and unknown voxels (unknown voxels come and go next to the border:
    the inner-voxel rule of SetUncertainToUnknown); then three overlapping edits one after another."""
    cfg = default_map_config(voxel_size=0.3, inflation_dist=setting[0], potential_dist=setting[1], potential_pow=setting[2])
    rng = np.random.default_rng(7 + int(100 * setting[0] + 10 * setting[1]))
    full = lambda raw: hdsm.map_preprocess(cfg, raw[None])[0]
    n_checked = n_changed = 0
    for shape in ((23, 37, 40), (6, 9, 13)):
        raw = wu.random_raw(rng, shape, p_occ=0.02, p_unk=0.03)
        old = full(raw)
        for t, (lo, bd) in enumerate(_boxes(shape[::-1])):
            edits = [wu.random_edit(rng, raw, lo, bd)]
            if t >= 5:  # corners and faces
                edits += [_fill(raw, lo, bd, 100), _fill(raw, lo, bd, 0), _fill(raw, lo, bd, -1)]
            for e, edited in enumerate(edits):
                got, want = hdsm.map_preprocess_region(cfg, edited, old, lo, bd), full(edited)
                assert np.array_equal(got, want), (shape, lo, bd, e, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
                n_checked += 1
                n_changed += int((want != old).any())
        cur_raw, cur = raw, old
        for step in range(3):  # a sequence: each edit starts from what the one before left
            lo = [shape[2] // 2 - 2 + step, shape[1] // 2 - 1 + step, max(0, shape[0] // 2 - 2 + step)]
            bd = [4, 3, min(3, shape[0] - lo[2])]
            cur_raw = wu.random_edit(rng, cur_raw, lo, bd)
            cur = hdsm.map_preprocess_region(cfg, cur_raw, cur, lo, bd)
            assert np.array_equal(cur, full(cur_raw)), (shape, "sequence", step)
            n_checked += 1
    assert n_checked >= 60 and n_changed > n_checked // 3


@pytest.mark.gpu
def test_region_preprocessing_on_narrow_boxes(hdsm):  # noqa: F811
    """Working boxes narrower than a quad. With every radius 0 the working box is the edit box itself, widened to four voxels where it
    holds fewer: a 1-voxel edit in the middle and in the far corner, a 3-wide edit (one quad), a 2-wide one ending at nx - 1 (rows of 3). With
    the shipped radii on grids 3, 2 and 1 voxels wide the working box is the whole grid and every row is shorter than a quad. Region
    == full grid on the whole array, bit for bit."""
    rng = np.random.default_rng(11)
    flat = default_map_config(voxel_size=0.3, inflation_dist=0.0, potential_dist=0.0, potential_pow=1)
    cases = [(flat, shape, lo, bd) for shape in ((23, 37, 40), (6, 9, 13))
             for lo, bd in (([shape[2] // 2, shape[1] // 2, shape[0] // 2], [1, 1, 1]), ([shape[2] - 1, shape[1] - 1, shape[0] - 1], [1, 1, 1]),
                            ([shape[2] // 2 - 1, 4, 2], [3, 1, 1]), ([shape[2] - 2, 0, 3], [2, 1, 1]), ([0, 0, 0], [1, 2, 1]))]
    shipped = default_map_config(**MAP_CFG)
    cases += [(shipped, shape, lo, bd) for shape in ((7, 5, 3), (5, 6, 2), (9, 4, 1))
              for lo, bd in (([0, 1, 2], [1, 1, 1]), ([shape[2] - 1, 2, 3], [1, 2, 2]), ([0, 0, 0], [shape[2], 1, 1]))]
    for cfg, shape, lo, bd in cases:
        raw = wu.random_raw(rng, shape, p_occ=0.05, p_unk=0.05)
        old = hdsm.map_preprocess(cfg, raw[None])[0]
        _, _, _, work = hdsm.map_region_extent(cfg, shape[::-1], lo, bd)
        assert int(np.prod(work)) >= 4 and (int(np.prod(work)) <= 6 if cfg is flat else int(work[0]) < 4)
        for value in (100, 0, -1):
            edited = _fill(raw, lo, bd, value)
            got, want = hdsm.map_preprocess_region(cfg, edited, old, lo, bd), hdsm.map_preprocess(cfg, edited[None])[0]
            assert np.array_equal(got, want), (shape, lo, bd, value, np.argwhere(got != want)[:4].tolist())


def _positions(dsw, loop):
    dsw.download(states=True)
    return loop.shard.state()[0]


def _edit_ahead(world, origin, pos, plans, agents, value=100):
    """2 x 2 columns over the whole height, five voxels ahead of the positions `pos` of `agents` (from the downloaded states; ahead =
    towards the end of the agent's plan) and two voxels to the side — inside what the decompositions seeded along their paths
    look at, beside what they fly: [(values, lo)]."""
    out = []
    for k in agents:
        h = (plans[k, -1, :3] - pos[k])[:2]
        nrm = np.linalg.norm(h)
        h = h / nrm if nrm > 1e-9 else np.array([1.0, 0.0])
        v = np.floor((np.r_[pos[k][:2] + h * 1.5 + np.array([-h[1], h[0]]) * 0.6, 0.0] - origin) / 0.3).astype(int)
        lo = [int(np.clip(v[0], 0, world.shape[2] - 2)), int(np.clip(v[1], 0, world.shape[1] - 2)), 0]
        out.append((np.full((world.shape[0], 2, 2), value, np.int8), lo))
    return out


def _free_a_pillar(world, pick):
    """A 5 x 5 column of free voxels round an occupied voxel of the world (one pillar goes): (values, lo)."""
    occ = np.argwhere(world[world.shape[0] // 2] >= 100)
    j, i = occ[pick % len(occ)]
    lo = [max(0, int(i) - 2), max(0, int(j) - 2), 0]
    return np.zeros((world.shape[0], min(5, world.shape[1] - lo[1]), min(5, world.shape[2] - lo[0])), np.int8), lo


def _world_of(n_rob, seed=21):
    raw, origin = sc.forest_for_circle(n_rob, seed=seed)
    return raw, sc.inflate(raw), origin


@pytest.mark.gpu
def test_device_loop_follows_the_host_mirror_across_edits(hdsm):  # noqa: F811
    """48 agents in the forest, a path period of 1. Ten rounds (the polyhedron cache is serving hits), then pillars appear a few voxels
    ahead of twelve agents (positions from the downloaded states) and a pillar goes elsewhere, through update_world on both sides;
    15 more rounds agree like the rounds before (statuses, flags, plans to 1e-7: tests/test_gpu_path_replanning.py), the corridor
    codes too; a second edit, ten more rounds. Without the k_cache_invalidate launch the device corridor forms polyhedra from
    structures grown in the old world, and this test fails in the first round after the first
    edit, with plans 0.13 apart."""
    from multi_agent_pkgs_amd import swarm
    (_, host), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1)
    _, world, origin = _world_of(48)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    assert dsw.world_stats() == {"updates": 0, "voxels": 0, "dropped": 0, "raw_resident": False}
    for r in range(10):
        _compare(host, dsw, r)
    cs = dsw.cache_stats()
    assert cs["cache_on"] and cs["hits_same_grid"] + cs["hits_interior"] > 0, cs
    r0, written = 10, 0
    for stage, (agents, rounds) in enumerate(((range(0, 48, 4), 15), (range(2, 48, 6), 10))):
        plans, pos = dsw.download(states=False)[0], _positions(dsw, dev_loop)
        edits = _edit_ahead(world, origin, pos, plans, agents) + [_free_a_pillar(world, 7 + 31 * stage)]
        for vals, lo in edits:
            world[:, lo[1]:lo[1] + vals.shape[1], lo[0]:lo[0] + vals.shape[2]] = vals
            host.update_world(vals, lo)
            dsw.update_world(vals, lo)
            written += vals.size
        assert np.array_equal(dsw.download_world(), world)
        for r in range(r0, r0 + rounds):
            _compare(host, dsw, r)
            dsw.download(states=True)
            assert (dev_loop.shard.corridor_errors()[1] == host.shard.corridor_errors()[1]).all(), r
        r0 += rounds
        ws = dsw.world_stats()
        assert ws["updates"] == (13 if stage == 0 else 13 + 9) and ws["voxels"] == written and ws["dropped"] > 0, ws
    assert dsw.cache_stats()["hits_same_grid"] + dsw.cache_stats()["hits_interior"] > cs["hits_same_grid"] + cs["hits_interior"]
    dsw.close()


@pytest.mark.gpu
def test_raw_world_updates_on_the_device(hdsm):  # noqa: F811
    """set_raw_world, then raw edits — through the host-pointer form and through the device-pointer form on the stream the rounds
    run on. After each the device world is hdsm_map_preprocess of the edited raw grid bit for bit, and the flight equals a
    host mirror that is given the processed voxels of W through update_world."""
    import torch
    from multi_agent_pkgs_amd import swarm
    (_, host), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1)
    raw, _, origin = _world_of(48)
    cfg = default_map_config(**MAP_CFG)
    full = lambda g: hdsm.map_preprocess(cfg, g[None])[0]
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    st = torch.cuda.Stream()
    with pytest.raises(hdsm.HdsmError) as e:
        dsw.update_world_raw(np.zeros((1, 1, 1), np.int8), [0, 0, 0])       # no raw world yet
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    dsw.set_raw_world(cfg, raw)
    world = full(raw)
    assert np.array_equal(dsw.download_world(), world) and dsw.world_stats()["raw_resident"]
    host.shard.set_world(world, origin)

    def fly(r0, n):
        for r in range(r0, r0 + n):
            out = host.step()
            dsw.round(stream=st)
            plans, has, status, _ = dsw.download(states=False)
            assert (has == host.has_plan).all() and (status == out["status"]).all(), r
            assert np.abs(plans - host.plans_all).max() < 1e-7, (r, float(np.abs(plans - host.plans_all).max()))

    fly(0, 6)
    keep = []
    for stage in range(2):
        plans, pos = dsw.download(states=False)[0], _positions(dsw, dev_loop)
        (vals, lo), = _edit_ahead(raw, origin, pos, plans, [5 + 20 * stage])
        if stage == 1:                                                   # (before the second one a pillar goes, through the host form)
            fv, flo = _free_a_pillar(raw, 11)
            raw[:, flo[1]:flo[1] + fv.shape[1], flo[0]:flo[0] + fv.shape[2]] = fv
            dsw.update_world_raw(fv, flo)
        raw[:, lo[1]:lo[1] + 2, lo[0]:lo[0] + 2] = vals
        if stage == 0:
            dsw.update_world_raw(vals, lo)
        else:
            keep.append(torch.from_numpy(vals).cuda())
            dsw.update_world_raw(keep[-1], lo, stream=st)
        new = full(raw)
        assert np.array_equal(dsw.download_world(), new), (stage, int((dsw.download_world() != new).sum()))
        diff = np.argwhere(new != world)
        assert len(diff)
        dlo, dhi = diff.min(0), diff.max(0) + 1                          # [z, y, x]
        host.update_world(new[dlo[0]:dhi[0], dlo[1]:dhi[1], dlo[2]:dhi[2]], dlo[::-1])
        world = new
        fly(6 + 5 * stage, 5)
    ws = dsw.world_stats()
    assert ws["updates"] == 3 and ws["dropped"] > 0 and ws["raw_resident"], ws
    dsw.close()


@pytest.mark.gpu
def test_an_edit_far_from_every_agent_drops_nothing(hdsm):  # noqa: F811
    """Selectivity: twin flights; after ten rounds one of them takes an edit in the corner of the world, further from every agent than
    the local grid's half width plus what an invalidation looks at. No cache entry is dropped and the next rounds' cache counters
    grow exactly as the twin's."""
    from multi_agent_pkgs_amd import swarm
    (sol_a, loop_a), (sol_b, loop_b) = forest_pair(hdsm, 48, 1)
    _, world, origin = _world_of(48)
    a, b = swarm.DeviceSwarm(loop_a.shard, sol_a), swarm.DeviceSwarm(loop_b.shard, sol_b)
    for r in range(10):
        a.round(), b.round()
    ca, cb = a.cache_stats(), b.cache_stats()
    assert ca["hits_same_grid"] + ca["hits_interior"] > 0
    grown = lambda now, then: {k: now[k] - then[k] for k in ("asked", "hits_same_grid", "hits_interior")}
    v = np.floor((_positions(a, loop_a) - origin) / 0.3).astype(int)
    lo, vals = [0, 0, 0], np.full((world.shape[0], 3, 3), 100, np.int8)
    # every seed lies in its agent's local grid (66 voxels wide in x and y, the agent in the middle)
    assert np.max(np.abs(v[:, :2] - 2), axis=1).min() > 33 + LOOK + 3
    a.update_world(vals, lo)
    ws = a.world_stats()
    assert ws["updates"] == 1 and ws["voxels"] == vals.size and ws["dropped"] == 0, ws
    for r in range(3):
        a.round(), b.round()
        assert grown(a.cache_stats(), ca) == grown(b.cache_stats(), cb), r
    assert a.cache_stats()["asked"] > ca["asked"]
    # ... and an edit that covers the world drops every entry there is
    a.update_world(world, [0, 0, 0])
    assert a.world_stats()["dropped"] >= 48
    a.close(), b.close()


@pytest.mark.gpu
def test_takeover_after_edits(hdsm):  # noqa: F811
    """A dswarm that took edits is downloaded — states, plans, and the device world into its mirror — and created again: the new one
    goes on like the host mirror that was kept in step, for 5 rounds."""
    from multi_agent_pkgs_amd import swarm
    (_, host), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1)
    _, world, origin = _world_of(48)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    for r in range(6):
        _compare(host, dsw, r)
    plans, pos = dsw.download(states=False)[0], _positions(dsw, dev_loop)
    for vals, lo in _edit_ahead(world, origin, pos, plans, range(1, 48, 5)) + [_free_a_pillar(world, 3)]:
        world[:, lo[1]:lo[1] + vals.shape[1], lo[0]:lo[0] + vals.shape[2]] = vals
        host.update_world(vals, lo)
        dsw.update_world(vals, lo)
    for r in range(6, 10):
        _compare(host, dsw, r)
    plans, has, _, _ = dsw.download(states=True)
    dev_loop.shard.set_world(dsw.download_world(), origin)
    dsw.close()
    dsw2 = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    dsw2.upload_plans(plans, has)
    assert np.array_equal(dsw2.download_world(), world)
    for r in range(10, 15):
        _compare(host, dsw2, r)
    dsw2.close()


@pytest.mark.gpu
def test_device_swarm_lifecycle_with_every_option_on(hdsm):  # noqa: F811
    """Create / close three times in one process with every opt-in group of the device loop allocated: phase timing, the audit, a
    history of 4 rounds, a resident raw world. Each flight starts from the same untouched shard (nothing is downloaded into it),
    flies three rounds, takes one raw edit that writes a 2 x 2 column of the values already there, flies one more round, and is read
    out and closed before the next is made. The three flights agree — statuses and flags exactly, plans, every field of the flight
    record and the history rows to the tolerance of _compare — and each reports seven finite phase times, one update, a resident raw world.
    The three flights share one solver handle, which keeps every instance's last optimal working set as the seed of its next solve
    (hdsm_params.warm_start). Seeded with the sets of another flight's fourth round, round 2 of this flight ends for some agents in a
    different optimum of equal cost (every status is "proven optimal" either way): measured on the MI355X, flights 1 and 2 were then
    1.06 / 0.415 / 0.287 from flight 0 in the plans of rounds 2 / 3 / 4 (1.7e-13 in round 1), with and without the options, before and
    after DSwarm owned its memory by type; with the working sets forgotten before each flight, or with a fresh handle per flight, all
    four rounds agree bit for bit. So each flight starts from the same solver state too: reset_warm_start() before it is created."""
    from multi_agent_pkgs_amd import swarm
    (_, _), (sol_d, dev_loop) = forest_pair(hdsm, 48, 1)
    raw, _, _ = _world_of(48)
    assert raw.shape == (67, 240, 240) and raw.dtype == np.int8
    cfg = default_map_config(**MAP_CFG)
    lo = [100, 120, 0]
    column = raw[:, lo[1]:lo[1] + 2, lo[0]:lo[0] + 2].copy()
    flights = []
    for f in range(3):
        sol_d.reset_warm_start()
        dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
        dsw.set_phase_timing()
        dsw.set_audit()
        dsw.set_history(4)
        dsw.set_raw_world(cfg, raw)
        for r in range(3):
            dsw.round()
        dsw.update_world_raw(column, lo)
        dsw.round()
        plans, has, status, _ = dsw.download(states=False)
        out = dict(plans=plans, has=has, status=status, report=dsw.flight_report(), hist=dsw.history(mirror=False), phase=dsw.phase_ms(),
                   path_ms=dsw.last_path_ms(), audit_ms=dsw.last_audit_ms(), world=dsw.world_stats())
        dsw.close()
        assert len(out["phase"]) == 7 and np.isfinite(list(out["phase"].values())).all(), (f, out["phase"])
        assert np.isfinite([out["path_ms"], out["audit_ms"]]).all(), (f, out["path_ms"], out["audit_ms"])
        assert out["world"]["updates"] == 1 and out["world"]["raw_resident"], (f, out["world"])
        assert out["hist"][0].shape == (4, 48, 9) and out["hist"][1] == 0, f
        flights.append(out)
    first = flights[0]
    for f, out in enumerate(flights[1:], 1):
        assert (out["status"] == first["status"]).all() and (out["has"] == first["has"]).all(), f
        gap = lambda a, b: float(np.where(a == b, 0.0, np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))).max())  # (inf == inf: 0)
        apart = {"plans": gap(out["plans"], first["plans"]), "hist": gap(out["hist"][0], first["hist"][0])}
        for name in first["report"].dtype.names:
            apart["report." + name] = gap(out["report"][name], first["report"][name])
        print("flight", f, "apart from flight 0:", apart)
        assert max(apart.values()) < PLAN_TOL, (f, apart)


def test_world_update_kernels_use_no_scratch(tmp_path):
    """The kernels this feature adds — k_region_gather, k_region_scatter, the plain x pass k_pass<0, 0, 0, false> the region form
    starts with, k_box_put, k_cache_invalidate — ask for no private segment and spill no vector register."""
    import os

    assert os.path.exists(LIB), "libhdsm.so is not built"
    desc = _kernel_descriptors(tmp_path)
    for tag in ("15k_region_gather", "16k_region_scatter", "6k_passILi0ELi0ELi0ELb0EE", "9k_box_put", "18k_cache_invalidate"):
        mine = {k: v for k, v in desc.items() if tag in k}
        assert len(mine) == 1, (tag, sorted(mine))
        for k, v in mine.items():
            assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
            assert v["vgpr_count"] <= 128, (k, v)


@pytest.mark.gpu
def test_a_flight_without_map_updates_launches_nothing_new(hdsm):  # noqa: F811
    """Off means off: a flight that calls none of the new entry points books no update, no written voxel, no dropped entry and holds
    no raw world; the calls that need a world or a raw world refuse. (The kernels such a flight launches are listed in
    profiles/world_update_off_kernel_stats.csv: none of the new ones.)"""
    from multi_agent_pkgs_amd import swarm
    from multi_agent_pkgs_amd.params import agile_params
    (_, _), (sol_d, dev_loop) = forest_pair(hdsm, 16, 0)
    dsw = swarm.DeviceSwarm(dev_loop.shard, sol_d)
    for r in range(5):
        dsw.round()
    assert dsw.world_stats() == {"updates": 0, "voxels": 0, "dropped": 0, "raw_resident": False}
    one = np.zeros((1, 1, 1), np.int8)
    dsw.update_world(np.zeros((0, 1, 1), np.int8), [0, 0, 0])              # an empty box: a no-op
    for lo, shape in (([240, 0, 0], (1, 1, 1)), ([-1, 0, 0], (1, 1, 1)), ([239, 0, 0], (1, 1, 2)), ([0, 0, 66], (2, 1, 1))):
        with pytest.raises(hdsm.HdsmError) as e:
            dsw.update_world(np.zeros(shape, np.int8), lo)
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    assert dsw.world_stats()["updates"] == 0
    dsw.close()
    sol, loop = device_loop(hdsm, agile_params(10, max_rows_static=18), swarm.default_swarm_config(), 8)    # free space: no world
    free = swarm.DeviceSwarm(loop.shard, sol)
    for call in (lambda: free.update_world(one, [0, 0, 0]), lambda: free.set_raw_world(default_map_config(**MAP_CFG), one), free.download_world):
        with pytest.raises(hdsm.HdsmError) as e:
            call()
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG
    free.close()
