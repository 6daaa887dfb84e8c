"""The flight audit on the CPU (csrc/audit_core.h through hdsm_flight_audit_host and the host mirror): the host form against the
independent numpy restatement of audit_cases.py, the closed form against a dense sampling of t, the own-track rule against the
Python Raycast of test_host.py, the flight record of a flown swarm, the planner records, the argument checks and the resources of
the device kernels (read from the built code objects)."""
import ctypes as C

import numpy as np
import pytest

import audit_cases as ac
import dmp_cases as dc
from audit_cases import CLEAR, DBL_MAX, check_separation, check_track
from kernel_elf import LIB, _group_segments, _kernel_descriptors
from multi_agent_pkgs_amd import lib, swarm
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import agile_params

TIE_RATE = 0.02       # rows of a batch that may be closer than CLEAR


def check_sampling(rng, plans, has, S, r, z):
    """closed form <= sampled minimum (1001 samples of t), and sampled - closed <= |e|^2_w / (4 * 1000^2): the parabola's
    curvature times the square of half a sampling step. Both up to the rounding of one evaluation of q (ac.sampled_gap)."""
    n = plans.shape[0]
    if n <= 32:
        a, b = np.nonzero(~np.eye(n, dtype=bool))
        pairs = np.stack([a, b], axis=1)
    else:
        a = np.repeat(np.arange(n), 6)
        b = (a + rng.integers(1, n, a.size)) % n
        pairs = np.stack([a, b], axis=1)
    closed, sampled, ee, slack = ac.sampled_gap(plans, S, pairs, r, z)
    assert (closed <= sampled + slack).all(), float((closed - sampled).max())
    assert (sampled - closed <= ee / (4 * 1000.0 ** 2) + slack).all(), float((sampled - closed - ee / 4e6).max())
    return pairs.shape[0] * S


def test_host_form_equals_the_numpy_restatement_on_random_batches():
    """320 random batches (2..200 agents, step_plan 1 and 2, isotropic and anisotropic radii, random has_plan): sep2 to 1e-12,
    partner / sub-step exactly wherever numpy's runner-up is more than 1e-9 behind, at most 2 % of a batch's rows closer than that;
    the closed form is checked against 1001 samples of t on all pairs of a small batch and on six partners per agent of a large one."""
    rng = np.random.default_rng(2024)
    rows, unclear, sampled, seen = 0, 0, 0, set()
    for t in range(320):
        plans, has, S, (r, z) = ac.random_batch(rng, step_plan=1 + t % 2, aniso=bool((t // 2) % 2))
        n = plans.shape[0]
        got = lib.flight_audit_host(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z)
        u = check_separation(got, plans, has, S, 0, n, r, z)
        assert u <= TIE_RATE * n, (t, n, u)
        assert (got["occupied"] == 0).all() and (got["pot"] == 0).all() and (got["crossed"] == 0).all() and (got["unknown"] == 0).all()
        sampled += check_sampling(rng, plans, has, S, r, z)
        rows, unclear = rows + n, unclear + u
        seen.add((S, r == z))
    assert len(seen) == 4 and rows > 10000 and sampled > 100000
    print("rows", rows, "within 1e-9 of the runner-up", unclear, "pair sub-steps sampled", sampled)


def test_paths_that_cross_between_two_round_boundaries_are_seen():
    """Two agents 1.5 m apart at both ends of the step swap places: an end-point check reports sigma = 3, the audit the 0.1 m of
    the crossing (sigma = 0.2)."""
    plans, has = ac.crossing_pair()
    r = 0.25
    ends = np.linalg.norm(plans[0, :2, :3] - plans[1, :2, :3], axis=1) / (2 * r)
    assert ends.min() >= 3.0                                                   # what an end-point-only check sees: safe
    got = lib.flight_audit_host(plans, has, step_plan=1, drone_radius=r, drone_z_offset=r)
    sigma = np.sqrt(got["sep2"])
    assert (sigma < 1.0).all() and np.allclose(sigma, 0.1 / (2 * r), rtol=1e-12)
    assert got["partner"].tolist() == [1, 0] and (got["substep"] == 0).all()
    assert check_separation(got, plans, has, 1, 0, 2, r, r) == 0
    assert np.allclose(got["dist"], 1.5) and (got["speed"] == 0).all()


def test_named_separation_cases():
    r, z = 0.25, 0.4
    rng = np.random.default_rng(5)
    # coincident agents: q = 0
    p0 = np.array([[1.0, 2.0, 1.5], [1.0, 2.0, 1.5], [4.0, 2.0, 1.5]])
    st = np.tile(rng.integers(-4, 5, (1, ac.N_HOR, 3)) / 8.0, (3, 1, 1))         # (dyadic steps: every sum below is exact)
    plans, has = ac.records(p0, st), np.ones(3, np.uint8)
    got = lib.flight_audit_host(plans, has, step_plan=2, drone_radius=r, drone_z_offset=z)
    assert got["sep2"][:2].tolist() == [0.0, 0.0] and got["partner"][:2].tolist() == [1, 0] and (got["substep"][:2] == 0).all()
    # equal velocities (e = 0 exactly: no division): the ratio of the start, sub-step 0
    assert got["sep2"][2] == (3.0 * 3.0) / (2 * r) ** 2 and got["partner"][2] == 0
    # an exact tie: two partners mirrored about the subject, in either order of ids the lower one wins
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        p0 = np.zeros((3, 3))
        p0[order[0]], p0[order[1]], p0[order[2]] = [0, 0, 1.5], [0.75, 0, 1.5], [-0.75, 0, 1.5]
        st = np.zeros((3, ac.N_HOR, 3))
        st[order[1], :, 0], st[order[2], :, 0] = -0.125, 0.125
        got = lib.flight_audit_host(ac.records(p0, st), np.ones(3, np.uint8), step_plan=2, drone_radius=r, drone_z_offset=z)
        subj = order[0]
        assert got["partner"][subj] == min(order[1], order[2]) and got["substep"][subj] == 1
        assert got["sep2"][subj] == (0.5 * 0.5) / (2 * r) ** 2
    # a lone agent, and agents without a record are neither subjects nor partners
    plans, has, S, _ = ac.random_batch(rng, n=6, step_plan=1)
    has[:] = 0
    has[3] = 1
    got = lib.flight_audit_host(plans, has, step_plan=1, drone_radius=r, drone_z_offset=z)
    assert (got["sep2"] == DBL_MAX).all() and (got["partner"] == -1).all()
    assert got["dist"][3] > 0 and (np.delete(got["dist"], 3) == 0).all() and (np.delete(got["speed"], 3) == 0).all()
    # a subject window is a slice of the full result
    plans, has, S, _ = ac.random_batch(rng, n=90, step_plan=2)
    full = lib.flight_audit_host(plans, has, step_plan=2, drone_radius=r, drone_z_offset=z)
    for first, n_local in ((0, 30), (30, 30), (60, 30), (17, 1), (90, 0), (45, 45)):
        part = lib.flight_audit_host(plans, has, step_plan=2, first=first, n_local=n_local, drone_radius=r, drone_z_offset=z)
        assert part.tobytes() == full[first:first + n_local].tobytes()
        check_separation(part, plans, has, 2, first, n_local, r, z)


def own_track_worlds(map_preprocess):
    raw, origin = sc.forest_for_circle(48, seed=21)
    yield "forest", sc.inflate(raw), origin
    yield "preprocessed", dc.preprocessed(raw, map_preprocess), origin


def test_own_track_rule_follows_the_python_raycast_and_plain_look_ups(oracle):
    """cfg 3's inflated forest and the same forest through the map pre-processing (potential field, unknown voxels below the ground
    are not part of it): 640 tracks of two sub-steps — random, starting inside an obstacle, clipping a pillar between two free end
    points, leaving the world, running along a voxel face — compared exactly, doubles included (the same operations)."""
    rng = np.random.default_rng(77)
    total = dict(occupied=0, unknown=0, crossed=0, pot=0, tracks=0)
    for name, world, origin in own_track_worlds(oracle.map_preprocess):
        world = world.copy()
        world[:3][world[:3] == 0] = -1                                          # the three lowest layers unknown where they were free
        plans, has, S = ac.tracks_in_world(rng, world, origin, 320)
        got = lib.flight_audit_host(plans, has, step_plan=S, world=world, worigin=origin, voxel_size=0.3)
        want = check_track(got, plans, has, S, 0, 320, world, origin)
        clipped = (want["crossed"] > 0) & (want["occupied"] == 0)
        assert clipped.sum() >= 10, name                                        # a pillar clipped between free end points
        for f in ("occupied", "unknown", "crossed", "pot"):
            total[f] += int(want[f].sum())
        total["tracks"] += 320
        # free space: the voxel terms are 0, the lengths the same
        free = lib.flight_audit_host(plans, has, step_plan=S)
        assert (free["occupied"] == 0).all() and (free["crossed"] == 0).all() and np.array_equal(free["dist"], got["dist"])
    assert total["tracks"] >= 500 and all(total[f] > 0 for f in ("occupied", "unknown", "crossed", "pot")), total
    print(total)


def test_flight_record_of_the_eight_agent_exchange(oracle):
    """The 8-agent circular exchange of test_host.py flown with the audit on: the mirror's flight record equals the numpy
    restatement accumulated over the recorded plans of every round; the continuous sigma_min stays above 1 and no round is close."""
    prm = agile_params(10, max_rows_static=18)
    cfg = swarm.default_swarm_config()

    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"],
                             inp["A"], inp["b"], plans, has, n_threads=8)

    loop = swarm.SwarmLoop(prm, cfg, 8, solve=solve)
    with pytest.raises(lib.HdsmError):
        loop.shard.flight_report()                                              # never switched on: an error, not zeros
    loop.shard.set_audit(True)
    r, z, S = prm.drone_radius, prm.drone_z_offset, cfg.step_plan
    mine, ends, near_tie, flown, clear = ac.Flight(8, S), np.inf, 0, [], []
    for rd in range(100):
        loop.step()
        sep2, partner, substep, second, _ = ac.np_separation(loop.plans_all, loop.has_plan, S, 0, 8, r, z)
        mine.add(loop.has_plan, sep2, partner, substep, ac.np_track(loop.plans_all, loop.has_plan, S, 0, 8, None, None, 0.3, None))
        near_tie += int((second - sep2 <= CLEAR * sep2).sum())
        flown.append(loop.plans_all.copy()), clear.append(second - sep2 > CLEAR * sep2)
        pos = loop.plans_all[:, S, :3]
        ends = min(ends, (np.linalg.norm(pos[:, None] - pos[None], axis=2) + np.eye(8) * 1e9).min() / (2 * r))
    pos, dist, nfail = loop.shard.state()
    assert nfail.sum() == 0 and dist.max() < 0.2
    rep = loop.shard.flight_report()
    # The exchange is symmetric: an agent's two neighbours are equally far up to rounding in many rounds. The partner of the
    # minimum is compared exactly where numpy's runner-up (another partner) was more than 1e-9 behind in that round; elsewhere it
    # may be the runner-up, whose ratio in that round then is within 1e-9 of the minimum. Everything else is compared as it is.
    assert np.array_equal(rep["sep_round"], mine.sep_round)
    rep2 = rep.copy()
    for k in range(8):
        rd = int(mine.sep_round[k])
        if not clear[rd][k] and rep["sep_partner"][k] != mine.sep_partner[k]:
            q, _ = ac.pair_q(flown[rd][:, :S + 1, :3], np.array([k]), S, r, z)
            assert abs(q[0, :, rep["sep_partner"][k]].min() - mine.sep2_min[k]) <= CLEAR * mine.sep2_min[k]
            rep2["sep_partner"][k] = mine.sep_partner[k]
    assert mine.same_as(rep2) is None, mine.same_as(rep2)
    summ = swarm.flight_summary(rep)
    print("sigma_min continuous %.4f, end points only %.4f, rounds within 1e-9 of a tie %d" % (summ["sigma_min"], ends, near_tie), summ)
    assert summ["sigma_min"] > 1.0 and summ["close_rounds"] == 0 and (rep["close_rounds"] == 0).all()
    assert summ["sigma_min"] <= ends * (1 + 1e-12) and summ["rounds"] == 100 and summ["positions"] == 800
    assert summ["sigma_min"] == np.sqrt(rep["sep2_min"].min()) and summ["mean_potential"] == 0.0
    k = summ["sigma_min_agent"]
    assert rep["sep_partner"][k] == summ["sigma_min_partner"] and rep["sep_round"][k] == summ["sigma_min_round"]
    assert np.allclose(summ["mean_speed"], (rep["speed_sum"] / rep["rounds"]).mean())


def test_planner_records_are_unchanged_by_the_audit_and_arguments_are_checked(oracle, tmp_path):
    """state_hist_<id>.csv of a host flight is the same file with the audit on; the argument checks of the C ABI reach Python as
    HDSM_ERR_BAD_ARG."""
    prm = agile_params(10, max_rows_static=18)

    def cpu(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"],
                             plans, has, n_threads=4)

    L = lib.load()
    files = []
    for on in (False, True):
        loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), 4, solve=cpu)
        if on:
            loop.shard.set_audit(True, 1.2)
        for _ in range(5):
            loop.step()
        d = tmp_path / ("on" if on else "off")
        d.mkdir()
        buf = C.create_string_buffer(4096)
        assert L.hdsm_swarm_shutdown(loop.shard.h, 1, str(d).encode(), 1, buf, 4096) > 0
        files.append((d / "state_hist_1.csv").read_text())
        if on:
            rep = loop.shard.flight_report()
            assert (rep["rounds"] == 5).all() and (rep["positions"] == 5).all()
            plans, has = loop.plans_all, loop.has_plan
    assert files[0] == files[1] and len(files[0].strip().split("\n")) == 5

    def bad(fn, *a, **kw):
        with pytest.raises(lib.HdsmError) as e:
            fn(*a, **kw)
        assert e.value.code == lib.HDSM_ERR_BAD_ARG

    bad(lib.flight_audit_host, plans, has, drone_radius=0.0)
    bad(lib.flight_audit_host, plans, has, drone_z_offset=-0.25)
    bad(lib.flight_audit_host, plans, has, drone_radius=float("nan"))
    bad(lib.flight_audit_host, plans, has, step_plan=0)
    bad(lib.flight_audit_host, plans, has, step_plan=prm.n_hor + 1)
    bad(lib.flight_audit_host, plans, has, first=3, n_local=2)
    bad(lib.flight_audit_host, plans, has, world=np.zeros((4, 4, 4), np.int8), voxel_size=0.0)
    assert lib.flight_audit_host(plans, has, step_plan=prm.n_hor).shape == (4,)
    sh = swarm.SwarmShard(prm, swarm.default_swarm_config(), 4, 0, np.zeros((4, 3)), np.ones((4, 3)))
    bad(sh.flight_report)
    bad(sh.audit, plans, has)                                                   # the audit is off
    bad(sh.set_audit, True, 0.0)
    assert not sh.audit_on
    sh.set_audit(True)
    assert sh.audit_on
    bad(sh.audit, plans[:3], has[:3])
    sh.audit(plans, has)
    sh.set_audit(False)
    assert not sh.audit_on
    assert (sh.flight_report()["rounds"] == 1).all()                            # the record is kept when the audit is switched off


def test_audit_kernels_use_no_scratch_and_little_lds(tmp_path):
    """Every k_audit* kernel of the built library: no private segment, no spill, its own LDS within the 160 KB of a CU."""
    import os

    assert os.path.exists(LIB), "libhdsm.so is not built"
    desc = _kernel_descriptors(tmp_path)
    mine = {k: v for k, v in desc.items() if "k_audit" in k}
    assert {k[k.index("k_audit"):].split("E")[0] for k in mine} == {"k_audit", "k_audit_pack", "k_audit_track"}, sorted(mine)
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)
    lds = _group_segments(tmp_path)
    assert set(mine) <= set(lds), sorted(set(mine) - set(lds))
    for k in mine:
        assert lds[k] <= 160 * 1024, (k, lds[k])
    sweep = [k for k in mine if k[k.index("k_audit"):].split("E")[0] == "k_audit"]
    assert all(0 < lds[k] <= 8 * 1024 for k in sweep), {k: lds[k] for k in sweep}   # the partner tile: 64 partners x 4 positions x 3 doubles + ids
    print({k: dict(v, group_segment_fixed_size=lds[k]) for k, v in mine.items()})
