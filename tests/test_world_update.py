"""Map updates in flight, the part that needs no GPU: the locality of the map pre-processing (the radius claim the region form of
csrc/map_kernels.hip rests on) against the oracle's literal loops alone, the arithmetic of hdsm_map_region_extent, the host mirror's
hdsm_swarm_update_world against hdsm_swarm_set_world of the edited grid, and the argument errors."""
import ctypes as C
import math

import numpy as np
import pytest

import corridor_oracle as co
import path_cases as pc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params, default_map_config
from world_cases import SETTINGS, random_edit, random_raw

def radius(cfg):
    rn01 = math.ceil(cfg.inflation_dist / cfg.voxel_size)
    return 2 * rn01 + math.ceil(cfg.potential_dist / cfg.voxel_size)


def random_box(rng, shape, max_side=6):
    nz, ny, nx = shape
    bdim = [int(rng.integers(1, min(max_side, n) + 1)) for n in (nx, ny, nz)]
    lo = [int(rng.integers(0, n - b + 1)) for n, b in zip((nx, ny, nz), bdim)]
    return lo, bdim


def box_mask(shape, lo, dim):
    m = np.zeros(shape, bool)
    m[lo[2]:lo[2] + dim[2], lo[1]:lo[1] + dim[1], lo[0]:lo[0] + dim[0]] = True
    return m


@pytest.mark.parametrize("setting", SETTINGS)
def test_an_edit_changes_the_processed_grid_only_inside_the_write_box(oracle, setting):
    """Locality, against the oracle alone: the literal loops' result for the edited grid differs from that for the original one only
    inside the W hdsm_map_region_extent returns."""
    cfg = default_map_config(voxel_size=0.3, inflation_dist=setting[0], potential_dist=setting[1], potential_pow=setting[2])
    rng = np.random.default_rng(int(1000 * setting[0] + 10 * setting[1]) + setting[2])
    shape = (23, 37, 40)
    R = radius(cfg)
    spread = total = 0
    for case in range(6):
        raw = random_raw(rng, shape)
        before = oracle.map_preprocess(cfg, raw[None])[0]
        lo, bdim = random_box(rng, shape)
        edited = random_edit(rng, raw, lo, bdim)
        after = oracle.map_preprocess(cfg, edited[None])[0]
        wlo, wdim, _, _ = lib.map_region_extent(cfg, shape[::-1], lo, bdim)
        inside = box_mask(shape, wlo, wdim)
        assert not ((after != before) & ~inside).any(), (case, lo, bdim, np.argwhere((after != before) & ~inside)[:4])
        total += int((after != before).sum())
        spread += int(((after != before) & ~box_mask(shape, lo, bdim)).sum())
    assert total > 0
    assert spread > 0 or R == 0   # (the edits do reach beyond their own box: W is not checked on nothing)


def test_region_extent_arithmetic():
    """W = box (+) R and the working box = box (+) 2R, clipped at every face and corner; a one-voxel box; the whole grid; the widening
    of a working box of fewer than four voxels."""
    dim = (40, 37, 23)
    for setting in SETTINGS:
        cfg = default_map_config(voxel_size=0.3, inflation_dist=setting[0], potential_dist=setting[1], potential_pow=setting[2])
        R = radius(cfg)
        boxes = [([20, 18, 11], [1, 1, 1]), ([0, 0, 0], list(dim)), ([5, 30, 2], [3, 4, 5])]
        for ax in range(3):  # a box on each face ...
            for side in (0, 1):
                lo, bd = [20, 18, 11], [2, 3, 2]
                lo[ax] = 0 if side == 0 else dim[ax] - bd[ax]
                boxes.append((lo, bd))
        for corner in range(8):  # ... and in each corner
            bd = [2, 1, 3]
            boxes.append(([(dim[ax] - bd[ax]) if corner >> ax & 1 else 0 for ax in range(3)], bd))
        for lo, bd in boxes:
            wlo, wdim, blo, bdim = lib.map_region_extent(cfg, dim, lo, bd)
            for ax in range(3):
                assert wlo[ax] == max(0, lo[ax] - R) and wlo[ax] + wdim[ax] == min(dim[ax], lo[ax] + bd[ax] + R), (setting, lo, bd, ax)
                if int(np.prod([min(dim[a], lo[a] + bd[a] + 2 * R) - max(0, lo[a] - 2 * R) for a in range(3)])) >= 4:
                    assert blo[ax] == max(0, lo[ax] - 2 * R) and blo[ax] + bdim[ax] == min(dim[ax], lo[ax] + bd[ax] + 2 * R), (setting, lo, bd, ax)
                assert blo[ax] <= wlo[ax] and blo[ax] + bdim[ax] >= wlo[ax] + wdim[ax] and 0 <= blo[ax] and blo[ax] + bdim[ax] <= dim[ax]
            assert int(np.prod(bdim)) >= 4
    flat = default_map_config(voxel_size=0.3, inflation_dist=0.0, potential_dist=0.0, potential_pow=1)   # R = 0
    wlo, wdim, blo, bdim = lib.map_region_extent(flat, dim, [39, 36, 22], [1, 1, 1])
    assert list(wlo) == [39, 36, 22] and list(wdim) == [1, 1, 1] and int(np.prod(bdim)) >= 4
    assert all(blo[ax] <= wlo[ax] and blo[ax] + bdim[ax] == dim[ax] for ax in range(3))
    wlo, wdim, blo, bdim = lib.map_region_extent(flat, dim, [3, 4, 5], [0, 2, 2])    # an empty box: empty W
    assert int(np.prod(wdim)) == 0 and int(np.prod(bdim)) == 0


def _view(shard, k):
    P, RS = shard.prm.poly_hor, shard.prm.max_rows_static
    n_poly, rows = C.c_int32(), np.zeros(P, np.int32)
    A, b, seeds, pos = np.zeros((P, RS, 3)), np.zeros((P, RS)), np.zeros((P, 3)), np.zeros(3)
    d, i = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert shard.lib.hdsm_swarm_view(shard.h, k, None, None, None, None, None, 0, None, C.byref(n_poly), rows.ctypes.data_as(i), A.ctypes.data_as(d),
                                     b.ctypes.data_as(d), seeds.ctypes.data_as(d), pos.ctypes.data_as(d)) == 0
    return n_poly.value, rows, A, b, seeds, pos


def _pillar_ahead(world, origin, pos, heading, ahead=4, value=100):
    """A 2 x 2 column over the whole height, `ahead` voxels in front of `pos`: (values, lo) for update_world."""
    v = np.floor((pos + heading * ahead * 0.3 - origin) / 0.3).astype(int)
    lo = [int(np.clip(v[0], 0, world.shape[2] - 2)), int(np.clip(v[1], 0, world.shape[1] - 2)), 0]
    return np.full((world.shape[0], 2, 2), value, np.int8), lo


def test_host_mirror_update_world_equals_set_world_of_the_edited_grid(oracle):
    """Two forest mirrors fly the same rounds (the oracle solves); then one takes the edits through hdsm_swarm_update_world, the other
    the whole edited grid through hdsm_swarm_set_world. From then on: the same world inside the library, the same polyhedra after
    prepare_corridor bit for bit (hdsm_swarm_view), the same paths of the path step (period 1) and the same plans."""
    n = 10
    prm = agile_params(10, max_rows_static=18)
    raw, origin = sc.forest_for_circle(n, seed=21)
    world = sc.inflate(raw)

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has, n_threads=8)

    def make():
        loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), n, solve=cpu)
        loop.set_world(world, origin)
        loop.pmax = 49
        loop.shard.set_path_period(1)
        return loop

    a, b = make(), make()
    for r in range(3):
        a.step(), b.step()
    edited = world.copy()
    changed_polys = 0
    for stage in range(2):
        pos = a.shard.state()[0]
        goals = -pos  # (the circle exchange: everybody heads through the centre)
        for k in range(0, n, 3 if stage == 0 else 4):
            h = (goals[k] - pos[k]) / np.linalg.norm(goals[k] - pos[k])
            vals, lo = _pillar_ahead(edited, origin, pos[k], h, ahead=4 + stage)
            edited[:, lo[1]:lo[1] + 2, lo[0]:lo[0] + 2] = vals
            a.update_world(vals, lo)
        occ = np.argwhere(edited[5] >= 100)          # ... and a pillar goes: the occupied voxels round one of them are freed
        j, i = occ[len(occ) // (2 + stage)]
        lo = [max(0, int(i) - 2), max(0, int(j) - 2), 0]
        vals = np.zeros((edited.shape[0], 5, 5), np.int8)[:, : edited.shape[1] - lo[1], : edited.shape[2] - lo[0]]
        edited[:, lo[1]:lo[1] + vals.shape[1], lo[0]:lo[0] + vals.shape[2]] = vals
        a.update_world(vals, lo)
        b.shard.set_world(edited, origin)
        assert np.array_equal(co.export_agents(a.shard)[3], edited) and np.array_equal(co.export_agents(b.shard)[3], edited)
        for r in range(3):
            before = [_view(a.shard, k) for k in range(n)]
            a.shard.prepare_corridor(), b.shard.prepare_corridor()
            for k in range(n):
                va, vb = _view(a.shard, k), _view(b.shard, k)
                assert va[0] == vb[0] and all(np.array_equal(x, y) for x, y in zip(va[1:], vb[1:])), (stage, r, k)
                changed_polys += int(not np.array_equal(va[3], before[k][3]))
            assert (a.shard.corridor_errors()[1] == b.shard.corridor_errors()[1]).all()
            pa, na = a.shard.get_paths()
            pb, nb = b.shard.get_paths()
            assert np.array_equal(na, nb) and np.array_equal(pa, pb), (stage, r)
            # (the same round again through step(): prepare_corridor twice in a round changes nothing the two do not share)
            oa, ob = a.step(), b.step()
            assert (oa["status"] == ob["status"]).all() and np.array_equal(a.plans_all, b.plans_all), (stage, r)
    assert changed_polys > 0
    # hdsm_local_path_host on the world the edited mirror holds and on the edited grid itself
    wa = co.export_agents(a.shard)[3]
    cs = pc.make_cases(edited, origin, 60, np.random.default_rng(5))
    args = (pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
    ra, rb = lib.local_path_host(wa, *args, res=pc.VS), lib.local_path_host(edited, *args, res=pc.VS)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and (ra[2] == 0).any()


def test_update_world_in_the_mirror_is_seen_by_the_next_corridor():
    """The edit is not a no-op: a pillar put next to the path ahead of an agent at rest is cut out of the polyhedra its next corridor
    grows, and freeing it again gives the first corridor back."""
    prm = agile_params(10, max_rows_static=18)
    starts, goals = np.array([[0.0, 0.0, 1.5]]), np.array([[12.0, 0.0, 1.5]])
    origin = np.array([-15.0, -15.0, 0.0])
    world = np.zeros((20, 100, 140), np.int8)

    def corridor(edit):
        loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 1, starts=starts, goals=goals)
        loop.shard.set_world(world, origin)
        for vals, lo in edit:
            loop.update_world(vals, lo)
        loop.shard.prepare_corridor()
        return _view(loop.shard, 0)

    free = corridor([])
    lo, vals = [53, 52, 0], np.full((20, 2, 2), 100, np.int8)   # x in [0.9, 1.5], y in [0.6, 1.2]: ahead of the agent, beside its path
    cut = corridor([(vals, lo)])
    back = corridor([(vals, lo), (np.zeros_like(vals), lo)])
    assert free[0] >= 1 and cut[0] >= 1
    assert all(np.array_equal(x, y) for x, y in zip(free[1:], back[1:]))
    # the centres of the pillar's voxels lie inside a polyhedron of the free corridor and outside every polyhedron of the cut one
    holds = lambda v, p: any(all(v[2][j][r] @ p <= v[3][j][r] for r in range(v[1][j])) for j in range(v[0]))
    for i in (0, 1):
        for j in (0, 1):
            mid = np.array([origin[0] + (lo[0] + i + 0.5) * 0.3, origin[1] + (lo[1] + j + 0.5) * 0.3, 1.5])
            assert holds(free, mid) and not holds(cut, mid), (i, j)


def test_argument_errors():
    L = lib.load()
    cfg = default_map_config()
    i32 = lambda v: np.asarray(v, np.int32)
    for lo, bd in (([-1, 0, 0], [2, 2, 2]), ([0, 0, 0], [41, 1, 1]), ([39, 0, 0], [2, 1, 1]), ([0, 36, 0], [1, 2, 1]), ([0, 0, 23], [1, 1, 1]),
                   ([0, 0, 0], [1, -1, 1]), ([50, 0, 0], [0, 1, 1])):
        with pytest.raises(lib.HdsmError) as e:
            lib.map_region_extent(cfg, (40, 37, 23), lo, bd)
        assert e.value.code == lib.HDSM_ERR_BAD_ARG and "box" in str(e.value)
        assert L.hdsm_map_region_scratch_bytes(C.byref(cfg), lib._p(i32((40, 37, 23)), C.c_int32), lib._p(i32(lo), C.c_int32), lib._p(i32(bd), C.c_int32)) == 0
    with pytest.raises(lib.HdsmError):
        lib.map_region_extent(default_map_config(potential_dist=3.5), (40, 37, 23), [0, 0, 0], [1, 1, 1])   # rn2 = 12 > 9
    full = L.hdsm_map_region_scratch_bytes(C.byref(cfg), lib._p(i32((40, 37, 23)), C.c_int32), lib._p(i32([0, 0, 0]), C.c_int32), lib._p(i32((40, 37, 23)), C.c_int32))
    assert full == 4 * 40 * 37 * 23
    # the region pre-processing refuses the same boxes before it looks for a device
    g = np.zeros((23, 37, 40), np.int8)
    with pytest.raises(lib.HdsmError) as e:
        lib.map_preprocess_region(cfg, g, g, [38, 0, 0], [3, 1, 1])
    assert e.value.code == lib.HDSM_ERR_BAD_ARG
    assert np.array_equal(lib.map_preprocess_region(cfg, g, g + 7, [3, 3, 3], [0, 4, 4]), g + 7)   # an empty box: nothing happens, no device needed
    # the host mirror
    prm = agile_params(10, max_rows_static=18)
    loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 2)
    one = np.zeros((1, 1, 1), np.int8)
    with pytest.raises(lib.HdsmError) as e:
        loop.update_world(one, [0, 0, 0])                          # no world
    assert e.value.code == lib.HDSM_ERR_BAD_ARG
    loop.shard.set_world(np.zeros((6, 8, 10), np.int8), (0.0, 0.0, 0.0))
    loop.update_world(one, [9, 7, 5])
    loop.update_world(np.zeros((6, 8, 10), np.int8), [0, 0, 0])
    loop.update_world(np.zeros((0, 2, 2), np.int8), [0, 0, 0])     # empty: a no-op
    for lo, shape in (([10, 0, 0], (1, 1, 1)), ([0, 0, 0], (7, 1, 1)), ([-1, 0, 0], (1, 1, 1)), ([9, 7, 5], (1, 1, 2))):
        with pytest.raises(lib.HdsmError) as e:
            loop.update_world(np.zeros(shape, np.int8), lo)
        assert e.value.code == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_swarm_update_world(loop.shard.h, None, lib._p(i32([0, 0, 0]), C.c_int32), lib._p(i32([1, 1, 1]), C.c_int32)) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_swarm_update_world(None, None, None, None) == lib.HDSM_ERR_BAD_ARG
