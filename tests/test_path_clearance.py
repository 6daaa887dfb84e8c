"""The path step's clearance mode (csrc/path_core.h, 6a-7': the reference's distance-map planner and ShortenDMPPath) on the CPU:
hdsm_local_path_dmp_host against the independent restatement of dmp_cases.py, the optimality of its cost, what its segments cross,
the off switch, the host mirror and the new kernels' resources."""
import functools
import math

import numpy as np
import pytest

import dmp_cases as dc
import path_cases as pc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params

COUNTS = {"forest": 80, "fwf": 70, "halo40": 40, "halo41": 40}


@functools.lru_cache(maxsize=None)
def _results():
    """Per world: the cases, what the host form returns, what the restatement returns, what the plain step returns."""
    from oracle import pyoracle
    pyoracle.build()
    rng = np.random.default_rng(5)
    out = []
    for name, world, origin, sealed, blocks in dc.worlds(pyoracle.map_preprocess, halo_seeds=(40, 41)):
        n = COUNTS[name]
        cs = pc.make_cases(world, origin, n, rng, sealed=sealed, blocks=blocks)
        args = (world, pc.LDIM, cs["off"], cs["ground_k"], cs["origin"], cs["start"], cs["goal"])
        got = lib.local_path_dmp_host(*args, search_rad=dc.SEARCH_RAD, res=pc.VS)
        plain = lib.local_path_host(*args, res=pc.VS)
        want = [dc.plan(world, cs["off"][t], int(cs["ground_k"][t]), cs["origin"][t], cs["start"][t], cs["goal"][t]) for t in range(n)]
        out.append((name, world, cs, args, got, plain, want))
    return out


def test_host_form_equals_the_restatement_and_solves_its_share():
    """>= 200 cases in the pre-processed forest of cfg 3 and forest-wall-forest of cfg 5 and in halo worlds with sealed boxes and
    solid blocks: status, cost, n_raw, point count and every point bit for bit. Of the cases the plain step solves, at least half
    come back with status 0 (status 3 is the risk: ShortenDMPPath keeps the chain's voxels inside the potential field)."""
    total, kinds, plain_ok, both_ok = 0, set(), 0, 0
    for name, world, cs, args, (paths, n_path, status, cost, n_raw), plain, want in _results():
        for t, (w_st, w_pts, w_cost, w_raw, _) in enumerate(want):
            assert status[t] == w_st, (name, t, int(status[t]), w_st)
            assert cost[t] == w_cost and n_raw[t] == w_raw, (name, t, int(cost[t]), w_cost, int(n_raw[t]), w_raw)
            assert n_path[t] == len(w_pts), (name, t)
            if w_pts:
                assert np.array_equal(paths[t, : n_path[t]], np.array(w_pts)), (name, t, paths[t, : n_path[t]], w_pts)
            kinds.add(int(status[t]))
            rel = cs["goal"][t] - cs["origin"][t]
            if not ((rel > 0) & (rel < np.array(pc.LDIM) * pc.VS)).all():
                kinds.add("outside")
        total += len(want)
        plain_ok += int((plain[2] == 0).sum())
        both_ok += int(((plain[2] == 0) & (status == 0)).sum())
        print(name, "plain ok", int((plain[2] == 0).sum()), "clearance statuses", np.bincount(status, minlength=5).tolist(),
              "points median / max", int(np.median(n_path[status == 0])), int(n_path.max()))
    assert total >= 200
    assert {0, 1, 2, "outside"} <= kinds, kinds
    assert 2 * both_ok >= plain_ok, (both_ok, plain_ok)


def test_cost_is_the_optimum_over_the_tunnel_and_the_chain_has_less_potential():
    """Every case with status 0: the cost is the heapq Dijkstra's D(sv) over T and the chain realises it; the chain's summed
    potential is <= the BFS descent's (which lies in T and has the fewest hops), strictly lower in at least one case per world."""
    for name, world, cs, args, (paths, n_path, status, cost, n_raw), plain, want in _results():
        gains, checked = 0, 0
        for t in np.nonzero(status == 0)[0]:
            info = want[t][4]
            c, D, chain, prior = info["c"], info["D"], info["chain"], info["prior"]
            pot = lambda ch: sum(int(c[v[2], v[1], v[0]]) for v in ch)
            assert cost[t] == D[chain[0]] == pot(chain) + len(chain) - 1, (name, t)
            assert all(info["T"][v[2], v[1], v[0]] for v in prior), (name, t)
            assert len(chain) >= len(prior) and n_raw[t] == len(chain)
            assert cost[t] <= pot(prior) + len(prior) - 1
            assert pot(chain) <= pot(prior), (name, t, pot(chain), pot(prior))
            gains += pot(chain) < pot(prior)
            checked += 1
        print(name, "status 0:", checked, "strictly less potential:", gains)
        assert gains >= 1, name


def test_segments_are_free_and_shortcuts_cross_no_potential():
    """Every returned segment is free of occupied voxels; every segment that is not a consecutive pair of the raw path visits only
    voxels with c = 0 (the points Raycast visits, as ShortenDMPPath reads them)."""
    from refmath import py_raycast as _py_raycast
    shortcuts = 0
    for name, world, cs, args, (paths, n_path, status, cost, n_raw), plain, want in _results():
        for t in np.nonzero(status == 0)[0]:
            info = want[t][4]
            occ, val, raw = info["occ"], info["val"], info["raw"]
            origin = cs["origin"][t]
            vox = lambda p: np.floor((np.asarray(p) - origin) / pc.VS).astype(int)
            pts = paths[t, : n_path[t]]
            assert 2 <= len(pts) <= pc.PATH_PTS
            idx = [next(i for i, r in enumerate(raw) if np.array_equal(r, p)) for p in pts]
            assert idx == sorted(idx) and idx[0] == 0 and idx[-1] == len(raw) - 1
            s0 = vox(cs["start"][t])
            start_in_margin = bool(occ[s0[2], s0[1], s0[0]])  # (such a start leaves the margin on its first segment)
            for a, b, ia, ib in zip(pts[:-1], pts[1:], idx[:-1], idx[1:]):
                if not (start_in_margin and ia == 0):
                    m = max(1, int(np.ceil(np.linalg.norm(b - a) / (pc.VS / 4))))
                    for u in range(m + 1):
                        v = vox(a + (b - a) * (u / m))
                        assert not occ[v[2], v[1], v[0]], (name, t, a, b)
                if ib == ia + 1:
                    continue
                shortcuts += 1
                s, e = [(a[k] - origin[k]) / pc.VS for k in range(3)], [(b[k] - origin[k]) / pc.VS for k in range(3)]
                d = [s[k] - e[k] for k in range(3)]
                visited, hit = _py_raycast(val, pc.LDIM, s, e, math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                assert hit is None
                for p in visited + [s, e]:
                    i, j, k = int(p[0]), int(p[1]), int(p[2])
                    if 0 <= i < pc.LDIM[0] and 0 <= j < pc.LDIM[1] and 0 <= k < pc.LDIM[2]:
                        assert val(i, j, k) <= 0, (name, t, a, b, p)
    assert shortcuts > 100, shortcuts


def _forest_shards(n_rob=48, seed=21):
    from oracle import pyoracle
    pyoracle.build()
    prm = agile_params(10, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(n_rob)
    raw, origin = sc.forest_for_circle(n_rob, seed=seed)
    world = dc.preprocessed(raw, pyoracle.map_preprocess)

    def make():
        sh = swarm.SwarmShard(prm, cfg, n_rob, 0, starts, goals)
        sh.set_world(world, origin)
        return sh

    locs = [pc.local_grid(world, origin, s) for s in starts]
    args = (world, pc.LDIM, np.array([l[1] for l in locs]), np.array([l[2] for l in locs]), np.array([l[0] for l in locs]), starts, goals)
    return make, args


def test_off_switch_and_no_tunnel():
    """set_path_clearance(0) leaves the plain path step; search_rad < 0 (no tunnel) costs <= the 1.8 m tunnel, which costs <= the
    prior chain; radii beyond the mask are refused (swarm) / status 4 (batch)."""
    make, args = _forest_shards()
    plain, off = make(), make()
    off.set_path_clearance(1.8)
    off.set_path_clearance(0.0)
    assert plain.replan_paths() == off.replan_paths()
    (pp, pn), (op, on) = plain.get_paths(), off.get_paths()
    assert np.array_equal(pn, on) and np.array_equal(pp, op)
    hp, hn, hs = lib.local_path_host(*args, res=pc.VS, pmax=64)
    ok = hs == 0
    assert ok.sum() >= 24 and (off.path_errors()[1] == hs).all() and (plain.path_errors()[1] == hs).all()
    assert np.array_equal(hn[ok], pn[ok]) and np.array_equal(hp[ok], pp[ok])
    with pytest.raises(lib.HdsmError):
        off.set_path_clearance(16 * 0.3 + 0.1)
    with pytest.raises(lib.HdsmError):
        off.set_path_clearance(float("nan"))
    compared = 0
    for name, world, cs, a, (paths, n_path, status, cost, n_raw), _, want in _results()[:2]:
        sub = tuple(x[:30] if isinstance(x, np.ndarray) and x.shape[0] == len(status) else x for x in a[2:])
        _, _, st_all, cost_all, _ = lib.local_path_dmp_host(a[0], a[1], *sub, search_rad=-1.0, res=pc.VS)
        for t in range(30):
            if status[t] == 0 and st_all[t] == 0:
                info = want[t][4]
                prior_cost = sum(int(info["c"][v[2], v[1], v[0]]) for v in info["prior"]) + len(info["prior"]) - 1
                assert 0 <= cost_all[t] <= cost[t] <= prior_cost, (name, t, int(cost_all[t]), int(cost[t]), prior_cost)
                compared += 1
        assert (lib.local_path_dmp_host(a[0], a[1], *sub, search_rad=4.9, res=pc.VS)[2][status[:30] == 0] == 4).all()
    assert compared >= 20


def test_host_mirror_plans_in_clearance_mode():
    """set_path_clearance(1.8) and replan_paths() on a 48-agent forest: get_paths = hdsm_local_path_dmp_host on the agents' own
    problems; the plain step gives other paths there."""
    make, args = _forest_shards()
    sh = make()
    sh.set_path_clearance(1.8)
    failed = sh.replan_paths()
    paths, n_path = sh.get_paths()
    hp, hn, hs, hc, hr = lib.local_path_dmp_host(*args, search_rad=1.8, res=pc.VS, pmax=64)
    assert failed == int((hs != 0).sum()) and (sh.path_errors()[1] == hs).all()
    ok = hs == 0
    assert ok.sum() >= 24
    assert np.array_equal(n_path[ok], hn[ok]) and np.array_equal(paths[ok], hp[ok])
    assert (n_path[~ok] == 2).all()  # (a failed agent keeps its path: [start, goal])
    pp, pn, _ = lib.local_path_host(*args, res=pc.VS, pmax=64)
    assert not np.array_equal(pp[ok], hp[ok])


def test_clearance_kernels_have_no_scratch_and_fit_the_lds(tmp_path):
    """k_dmp and k_dmp_batch exist in the built library, use no scratch and at most 160 KB of LDS; no new symbol contains k_path
    (test_k_path_has_no_scratch_and_fits_two_workgroups_per_cu holds every *k_path* kernel to 80 KB)."""
    from kernel_elf import _kernel_blocks
    desc = _kernel_blocks(tmp_path)
    ks = {k: v for k, v in desc.items() if "k_dmp" in k}
    assert any("5k_dmpE" in k for k in ks) and any("11k_dmp_batchE" in k for k in ks), sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert 0 < v["group_segment_fixed_size"] <= 160 * 1024, (k, v)
    assert len([k for k in desc if "k_path" in k]) == 2, sorted(k for k in desc if "k_path" in k)
