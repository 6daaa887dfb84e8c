"""Row f1 off the device: the oracle's orc_reference against refmath.reference_row (long double, written from the reference's
text, no code shared with the oracle or the library) on every case of tests/reference_cases.py, and the conditions those cases
must meet for tests/test_gpu_reference_row.py to be able to see a failure — asserted from the rendering and from a host
restatement of the sphere test, never from the code under test.

Tolerance: the project's own for this row, 1e-10 * max(1, |y|.max()) per output (glibc's exp / pow against long double's differ by
an ulp or two of a number of a few units; the walk adds a few ulps of a coordinate below 100 m per step)."""
import math

import numpy as np
import pytest

import reference_cases as rc


def close(x, y, what):
    err, tol = np.abs(x - y).max(), 1e-10 * max(1.0, np.abs(y).max())
    assert err < tol, (what, err, tol)
    return err / max(1.0, np.abs(y).max())


def oracle_outputs(oracle, c):
    """orc_reference on the case; a grouped case as one call per id range with has_plan masked to it (the oracle knows no groups)"""
    N = c.n_hor
    full, ref, pv = np.zeros((c.n_inst, N + 1, 6)), np.zeros((c.n_inst, N, 6)), np.zeros(c.n_inst)
    for idx, mask in c.masked_calls():
        full[idx], ref[idx], pv[idx] = oracle.reference(c.prm(), c.cfg(), c.agent_id[idx], c.path[idx], c.n_path[idx], c.plans, mask,
                                                        vel_cap=None if c.caps is None else c.caps[idx])
    return full, ref, pv


@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_matches_the_long_double_rendering(oracle, name):
    c = rc.case(name)
    want = c.render()
    got = oracle_outputs(oracle, c)
    rel = [close(g, w, what) for g, w, what in zip(got, want, ("ref_full", "ref", "path_vel"))]
    if c.exact:
        assert got[2].tobytes() == want[2].tobytes() == c.caps.tobytes()
    print(f"{name}: NT = {c.nt}, largest relative difference {max(rel):.2e}")


def _setters(c):
    return np.array([f["setter"][0] if f["setter"] else -1 for f in c.render()[3]])


@pytest.mark.parametrize("name", [n for n in rc.names("capacity") if not n.startswith("sparse")])
def test_tight_ball_depends_on_both_sides_of_the_capacity(name):
    """A tight-ball case can only see a lost drain if path_vel depends on ids behind the list's capacity, and a lost first filling
    if it depends on ids before it: at least a tenth of the instances have their path_vel set by a neighbour below the capacity,
    and at least a tenth by one at or behind it (counted from the first id of the instance's range). Only with 2048 agents, where no
    id lies behind the capacity, is the second number 0. Where few ids lie behind it the cases are crafted: one id with 2049 agents
    (three clusters of twelve instances around the places agent 2048 visits), thirteen in the grouped range [70, 2131) (two
    instances beside each). And the list is filled: one instance at least keeps >= 2040 survivors among the first 2048 ids of its
    range."""
    c = rc.case(name)
    setter, rg = _setters(c), c.ranges()
    lo = np.zeros(c.n_inst, int) if rg is None else rg[:, 0]
    hi = np.full(c.n_inst, c.n_rob) if rg is None else rg[:, 1]
    above = (setter >= lo + rc.SURV_CAP).sum()
    below = ((setter >= 0) & (setter < lo + rc.SURV_CAP)).sum()
    tenth = math.ceil(0.1 * c.n_inst)
    need_above = tenth if (hi - lo > rc.SURV_CAP).any() else 0
    st = rc.sphere_stats(c)
    print(f"{name}: NT = {c.nt}, setters below / at or behind the capacity {below} / {above} of {c.n_inst} (needed {tenth} / {need_above}), "
          f"survivors min / median / max {st['survivors'].min()} / {np.median(st['survivors']):.0f} / {st['survivors'].max()}, "
          f"largest first filling {st['first_filling'].max()}")
    assert below >= tenth and above >= need_above
    assert st["first_filling"].max() >= 2040
    for k, nb in c.special.items():
        assert setter[k] == nb, (k, nb, setter[k])


@pytest.mark.parametrize("name", [n for n in rc.names("capacity") if n.startswith("sparse")])
def test_sparse_swarm_has_its_crafted_instances(name):
    """The instances whose only close neighbour is id 2047, 2048, n_rob - 1 have their path_vel set by that id; the instance of
    agent 0 has it set by agent 5 (a long plan, close at one late step) while the closest sphere is another agent's; the cull
    leaves few survivors."""
    c = rc.case(name)
    setter, st = _setters(c), rc.sphere_stats(c)
    for k, nb in c.special.items():
        assert setter[k] == nb, (k, nb, setter[k])
    k0 = int(np.nonzero(c.agent_id == 0)[0][0])
    assert c.special[k0] == 5 and st["jstar"][k0] not in (-1, 5) and c.render()[3][k0]["setter"][1] == c.n_hor - 1
    assert sorted(c.special.values())[-1] == c.n_rob - 1 and (2047 in c.special.values())
    assert st["survivors"].max() < 200
    print(f"{name}: NT = {c.nt}, survivors min / median / max {st['survivors'].min()} / {np.median(st['survivors']):.0f} / {st['survivors'].max()}")


def test_capacity_instances_are_a_shuffled_subset_with_the_ids_at_the_capacity():
    for name in rc.names("capacity"):
        c = rc.case(name)
        ids = c.agent_id.tolist()
        assert len(set(ids)) == c.n_inst < c.n_rob and ids != sorted(ids)
        assert {0, 2047, c.n_rob - 1} <= set(ids) and (c.n_rob == 2048 or 2048 in ids)


@pytest.mark.parametrize("name", rc.names("nonfinite"))
def test_non_finite_neighbour_sets_its_instance(name):
    """the plan that is non-finite (or, in case f, the one met after it) has has_plan = 1 and decides: without it the rendering's
    path_vel of its instance moves by more than 1e-6"""
    c = rc.case(name)
    (k, nb), = c.special.items()
    assert c.has_plan[nb] == 1 and c.has_plan[c.agent_id[k]] == 1
    assert not np.isfinite(c.plans[:, :, :3]).all()
    cleared = c.has_plan.copy()
    cleared[nb] = 0
    assert abs(c.render(only=[k], has_plan=cleared)[2][0] - c.render()[2][k]) > 1e-6
    assert c.render()[3][k]["setter"][0] == nb


@pytest.mark.parametrize("name", rc.NAMES)
def test_decision_margins(name):
    """under the case's vel_cap and under the other choice (the two calls of the GPU test):
    every comparison of the walk decides by more than 1e-7 and every 1e-2 test of the velocity row by more than 1e-6 — except in
    the exact-landing case, where every instance lands exactly (margin 0) and path_vel is the cap to the bit"""
    c = rc.case(name)
    info, pv = c.render()[3] + c.render(other=True)[3], c.render()[2]
    if c.exact:
        assert all(min(f["walk"]) == 0.0 for f in c.render()[3]) and all(f["setter"] is None for f in info)
        assert pv.tobytes() == c.caps.tobytes()
        return
    assert min(min(f["walk"], default=1.0) for f in info) > rc.WALK_MARGIN
    assert min(min(f["vel"], default=1.0) for f in info) > rc.VEL_MARGIN


def test_polyline_cases_cover_what_they_name():
    for name in rc.names("polyline"):
        c = rc.case(name)
        if c.exact:
            continue
        assert set(rc.N_PATHS) <= set(c.n_path.tolist()) and set(rc.CAPS) == set(c.caps.tolist()) and c.path.shape[1] == 80
        full, _, pv, info = c.render()
        crossed = [len(f["walk"]) - c.n_hor for f in info]             # path points passed inside the horizon
        assert max(crossed) >= 24 or c.cfg_kw["path_vel_dec"] == 100.0      # (a step clamped at 0 crosses nothing after the first)
        ended = [k for k in range(c.n_inst) if c.n_path[k] == 21 and (full[k, -1, :3] == c.path[k, 20]).all()]
        assert ended or c.cfg_kw["path_vel_dec"] == 100.0              # a path that runs out before the horizon
        assert any((c.path[k, 5] == c.path[k, 4]).all() for k in range(c.n_inst))
        assert any(0 < f["vel"][0] < 1e-2 and pv[k] > 0 for k, f in enumerate(info) if f["vel"])    # points closer than 1e-2 ...
        if c.cfg_kw["path_vel_dec"] == 100.0:                          # ... and the clamp of the step at 0
            assert any(pv[k] > 1.0 and (full[k, 1, :3] == full[k, -1, :3]).all() and c.n_path[k] == 80 for k in range(c.n_inst))
    c = rc.case("clamp")
    assert sorted(c.n_path_device.tolist())[:2] == [-3, 0] and c.n_path_device.max() == 85 and c.n_path_device[-1] <= 80
    over = np.nonzero(c.n_path_device > 80)[0]
    assert all((c.render()[0][k, -1, :3] == c.path[k, 79]).all() for k in over)     # the walk reaches the end of the polyline


def test_configuration_cases_cover_what_they_name():
    c = rc.case("plain-i300")
    assert (c.plans[5] == c.plans[6]).all() and c.has_plan[5] and c.has_plan[6]                    # coincident agents
    d8, d9 = (np.linalg.norm(c.plans[7, :, :3] - c.plans[j, :, :3], axis=1) for j in (8, 9))
    assert (d8 == d9).all()                                                                        # two neighbours equally far
    for name in rc.names("config"):
        c = rc.case(name)
        assert (c.has_plan[c.agent_id] == 0).any() and {1, 2, 5} <= set(c.n_path.tolist())
    c = rc.case("plain-i20-beyond")
    k = int(np.nonzero(c.agent_id == c.groups[-1] + 1)[0][0])
    assert c.n_rob == c.groups[-1] + 3 and c.render()[3][k]["setter"] is None
    assert (rc.case("sens_dist_negative-i300").render()[2] < 0).any()
