"""Formations on the CPU (csrc/assign_core.h, include/hdsm_swarm.h "formations"): hdsm_assign_host against the independent numpy
restatement of tests/assign_cases.py, exactly; optimality from the returned assignment and prices alone (permutation, duality gap,
brute force, scipy where it imports); the statuses; the argument checks; the host mirror's hdsm_swarm_assign."""
import numpy as np
import pytest

import assign_cases as ac
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import AssignSetting, agile_params

CASES = ac.cases()


@pytest.fixture(scope="module")
def host_results():
    """The host form on every case of the table, computed once."""
    return {case[0]: ac.run(case) for case in CASES}


def _same(got, want, name):
    assert np.array_equal(got[0], want[0]), (name, "slot_of")
    assert np.array_equal(got[1], want[1]), (name, "price")
    for field in ("first", "count", "active", "status", "phases", "iters", "bids", "cost", "reserved0"):
        assert np.array_equal(got[2][field], want[2][field]), (name, field, got[2][field][:8], want[2][field][:8])


def test_the_host_form_equals_the_restatement_on_every_case(host_results):
    seen = set()
    for case in CASES:
        name, pos, slots, groups, active = case
        got = host_results[name]
        _same(got, ac.solve(pos, slots, groups, active), name)
        seen |= set(got[2]["status"].tolist())
        seen.add("inactive" if (got[0] == -1).any() else "all")
        seen.add("empty group" if (got[2]["active"] == 0).any() else "groups")
    assert {0, 2, "inactive", "empty group"} <= seen, seen       # what the cases are there for did happen
    by_name = {c[0]: host_results[c[0]] for c in CASES}
    assert by_name["a circle against its antipodal roll"][2]["cost"][0] == 0
    assert by_name["everything at the origin"][2]["cost"][0] == 0 and by_name["everything at the origin"][2]["phases"][0] == 1
    _, pos, slots, _, _ = next(c for c in CASES if c[0] == "a cloud 10 km wide")
    assert (ac.cost_matrix(pos, slots) == ac.COST_CAP).any()     # (the clamp is met)


def test_the_assignment_is_optimal_by_its_own_certificate(host_results):
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    brute = 0
    for name, pos, slots, groups, active in CASES:
        slot_of, price, stats = host_results[name]
        act = np.ones(len(pos), bool) if active is None else active != 0
        assert (slot_of[~act] == -1).all() and (price[~act] == 0).all(), name
        for g, (lo, hi) in enumerate(ac.partition(len(pos), groups)):
            idx = lo + np.nonzero(act[lo:hi])[0]
            m = len(idx)
            assert stats[g]["active"] == m and (stats[g]["first"], stats[g]["count"]) == (lo, hi - lo), (name, g)
            if m == 0:
                assert stats[g]["status"] == 0 and stats[g]["iters"] == 0
                continue
            assert sorted(slot_of[idx].tolist()) == idx.tolist(), (name, g)              # a permutation of the group's own slots
            if stats[g]["status"] != 0:
                continue
            c = ac.cost_matrix(pos[idx], slots[idx])
            has = np.searchsorted(idx, slot_of[idx])
            cost = int(c[np.arange(m), has].sum())
            assert cost == stats[g]["cost"], (name, g)
            gap = ac.duality_gap(c, has, price[idx])
            assert 0 <= gap <= m, (name, g, gap)
            if m <= 7:
                assert cost == ac.brute_force_cost(c), (name, g)
                brute += 1
            if linear_sum_assignment is not None:
                r, k = linear_sum_assignment(c)
                assert cost == int(c[r, k].sum()), (name, g)
    assert brute > 250


def test_a_budget_that_runs_out_a_position_not_finite_and_a_bid_too_high_give_the_identity(monkeypatch):
    rng = np.random.default_rng(5)
    pos, slots = rng.uniform(0, 60, (12, 3)), rng.uniform(0, 60, (12, 3))
    groups = [0, 5, 12]
    ident = np.arange(12)
    slot_of, price, stats = lib.assign(pos, slots, groups=groups, setting=AssignSetting(max_iters=1))
    assert stats["status"].tolist() == [1, 1] and np.array_equal(slot_of, ident) and not price.any()
    assert stats["iters"].tolist() == [1, 1] and stats["bids"].tolist() == [5, 7] and not stats["cost"].any() and not stats["phases"].any()
    _same((slot_of, price, stats), ac.solve(pos, slots, groups, max_iters=1), "budget")
    # a budget of exactly the iterations a group needs is enough; one fewer is not
    free = lib.assign(pos, slots, groups=groups)
    need = free[2]["iters"].astype(int)
    assert lib.assign(pos, slots, groups=groups, setting=AssignSetting(max_iters=int(need.max())))[2]["status"].tolist() == [0, 0]
    short = lib.assign(pos, slots, groups=groups, setting=AssignSetting(max_iters=int(need.max()) - 1))[2]["status"]
    assert short.tolist() == [int(need[0] == need.max()), int(need[1] == need.max())]
    bad = pos.copy()
    bad[8, 0] = -np.inf
    slot_of, price, stats = lib.assign(bad, slots, groups=groups)
    assert stats["status"].tolist() == [0, 2] and np.array_equal(slot_of[5:], ident[5:]) and not price[5:].any()
    assert np.array_equal(slot_of[:5], free[0][:5]) and np.array_equal(price[:5], free[1][:5])
    # No input reaches a bid of 2^52 (costs end at 2^34, m + 1 at 1025, and a price rises by no more than the benefits' range and
    # eps per phase): the library's test hook lowers the limit for the host form and the device alike, the restatement takes it as
    # an argument.
    monkeypatch.setenv("HDSM_ASSIGN_BID_LIMIT_LOG2", "24")
    got = lib.assign(pos, slots, groups=groups)
    monkeypatch.delenv("HDSM_ASSIGN_BID_LIMIT_LOG2")
    assert got[2]["status"].tolist() == [3, 3] and np.array_equal(got[0], ident) and not got[1].any()
    _same(got, ac.solve(pos, slots, groups, bid_limit=2 ** 24), "bid limit")
    _same(lib.assign(pos, slots, groups=groups), free, "the hook is read at every call")


def test_arguments_out_of_bounds_are_refused_with_nothing_changed():
    L = lib.load()
    rng = np.random.default_rng(9)
    n = 6
    pos, slots = rng.uniform(0, 9, (n, 3)), rng.uniform(0, 9, (n, 3))
    good = dict(setting=AssignSetting(), n=n, n_groups=2, gs=np.array([0, 2, 6], np.int32), pos=pos, active=None, slots=slots)
    nan_slots, inf_slots = slots.copy(), slots.copy()
    nan_slots[3, 1], inf_slots[0, 2] = np.nan, np.inf
    bad = [dict(n=-1), dict(gs=np.array([1, 2, 6], np.int32)), dict(gs=np.array([0, 2, 5], np.int32)), dict(gs=np.array([0, 3, 3, 6], np.int32), n_groups=3),
           dict(gs=np.array([0, 4, 2, 6], np.int32), n_groups=3), dict(n_groups=-1), dict(slots=nan_slots), dict(slots=inf_slots), dict(pos=None), dict(slots=None),
           dict(setting=AssignSetting(quantum=0.0)), dict(setting=AssignSetting(quantum=-0.01)), dict(setting=AssignSetting(quantum=float("nan"))),
           dict(setting=AssignSetting(quantum=float("inf"))), dict(setting=AssignSetting(quantum=1e-200)), dict(setting=AssignSetting(max_iters=-1))]
    for over in bad:
        a = dict(good, **over)
        slot_of, price, stats = np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.zeros(3, lib.ASSIGN_STATS)
        stats["status"] = -7
        rc = L.hdsm_assign_host(a["setting"], a["n"], a["n_groups"], a["gs"], a["pos"], a["active"], a["slots"], slot_of, price, stats)
        assert rc == lib.HDSM_ERR_BAD_ARG, over
        assert (slot_of == -7).all() and (price == -7).all() and (stats["status"] == -7).all(), over
    assert L.hdsm_assign_host(good["setting"], n, 2, good["gs"], pos, None, slots, None, None, None) == lib.HDSM_ERR_BAD_ARG
    # more than HDSM_ASSIGN_MAX active agents in one group; with one of them inactive it fits
    big = lib.ASSIGN_MAX + 1
    z, slot_of = np.zeros((big, 3)), np.full(big, -7, np.int32)
    assert L.hdsm_assign_host(None, big, 0, None, z, None, z, slot_of, None, None) == lib.HDSM_ERR_CAPACITY and (slot_of == -7).all()
    active = np.ones(big, np.uint8)
    active[11] = 0
    assert L.hdsm_assign_host(None, big, 0, None, z, active, z, slot_of, None, None) == 0 and slot_of[11] == -1 and (np.delete(slot_of, 11) >= 0).all()
    # a NULL setting is the default setting; price and stats may be NULL; n = 0 is legal
    a, b = lib.assign(pos, slots, setting=None), lib.assign(pos, slots, setting=AssignSetting(0.01, 0))
    _same(a, b, "defaults")
    assert L.hdsm_assign_host(None, 0, 0, None, None, None, None, None, None, None) == 0
    with pytest.raises(lib.HdsmError) as e:
        lib.assign(pos, slots, groups=[0, 7])
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: hdsm_assign_host"


# ---- the host mirror ----
def _shard(starts, groups=None):
    shard = swarm.SwarmShard(agile_params(10, max_rows_static=18), swarm.default_swarm_config(), len(starts), 0, starts, starts + [0.0, 0.5, 0.0])
    if groups is not None:
        shard.set_groups(groups)
    return shard


@pytest.mark.parametrize("groups", [None, [0, 3, 9]])
def test_the_mirror_applies_an_assignment_exactly_as_set_goals_would(groups):
    rng = np.random.default_rng(3)
    starts = sc.grid_formation(9, pitch=2.0)
    slots = sc.line_formation(9, pitch=2.0, origin=(12.0, 4.0, 1.5))[rng.permutation(9)]
    slots[4] = starts[4] + [0.0, 0.5, 0.0]             # (a slot that IS somebody's current goal: that agent may not become due)
    a, b = _shard(starts, groups), _shard(starts, groups)
    want = lib.assign(starts, slots, groups=groups)
    slot_of, stats = a.assign(slots, apply=False)
    assert np.array_equal(slot_of, want[0]) and stats.tobytes() == want[2].tobytes()
    due, goals = a.mission_due()
    assert not due.any() and np.array_equal(goals, starts + [0.0, 0.5, 0.0])      # apply = 0 touches nothing
    slot_of, _ = a.assign(slots, apply=True)
    b.set_goals(slots[want[0]])
    (due_a, goals_a), (due_b, goals_b) = a.mission_due(), b.mission_due()
    assert np.array_equal(goals_a, slots[slot_of]) and np.array_equal(goals_a, goals_b) and np.array_equal(due_a, due_b)
    assert due_a.sum() >= 8
    # under a mission apply = 1 is refused with nothing changed, apply = 0 is not
    a.set_mission(sc.mission_setting(1), starts[:, None, :] + [1.0, 0.0, 0.0])
    before = a.mission_due()
    with pytest.raises(lib.HdsmError) as e:
        a.assign(slots[::-1].copy(), apply=True)
    assert e.value.code == lib.HDSM_ERR_BAD_ARG
    after = a.mission_due()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(a.assign(slots, apply=False)[0], want[0])
    # slots that are not finite, and a shard that is not the whole swarm
    bad = slots.copy()
    bad[2, 2] = np.nan
    with pytest.raises(lib.HdsmError):
        b.assign(bad, apply=False)
    part = swarm.SwarmShard(agile_params(10, max_rows_static=18), swarm.default_swarm_config(), 9, 3, starts[3:6], starts[3:6])
    with pytest.raises(lib.HdsmError):
        part.assign(slots[:3], apply=False)


def test_the_formations_have_their_shapes():
    for n in (1, 2, 7, 16, 17):
        for f in (sc.line_formation(n), sc.circle_formation(n), sc.grid_formation(n)):
            assert f.shape == (n, 3) and f.dtype == np.float64 and np.isfinite(f).all()
            if n > 1:
                d = np.linalg.norm(f[:, None] - f[None], axis=2) + np.eye(n) * 9.0
                assert d.min() > 1.99, (n, d.min())                                # nobody closer than the pitch
    assert np.allclose(sc.grid_formation(7, pitch=1.0, origin=(0, 0, 0), columns=3)[[0, 2, 3, 6]], [[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 2, 0]])
    assert np.allclose(sc.line_formation(3, pitch=2.0, origin=(1, 1, 1), direction=(3, 0, 0)), [[1, 1, 1], [3, 1, 1], [5, 1, 1]])
