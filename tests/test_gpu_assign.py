"""Formations on the MI355X (hdsm_assign_batch, hdsm_dswarm_assign, k_assign, swarm.fly_formations; include/hdsm_swarm.h
"formations"):

  * batch equals host: hdsm_assign_batch equals hdsm_assign_host bit for bit on the whole table of tests/assign_cases.py, at m = 1023 and
    1024, with groups of 64 and 65 in one launch (one and two wavefronts per workgroup), under every status, and the capacity error;
  * the device loop: after a few rounds of an 8-agent flight and of a 66-agent grouped flight hdsm_dswarm_assign equals the host form on
    the states the harness downloads; apply = 0 changes nothing on the device; apply = 1 leaves exactly the goals and due agents of
    set_goals, the next round's path step counts them, and the flight stays with the host mirror given the same call; a scripted tail
    keeps -1; a mission refuses apply = 1 and allows apply = 0;
  * fly_formations: a small lattice flies line to grid to line, every summary ends with done == flown;
  * resources: k_assign uses no scratch."""
import numpy as np
import pytest

import assign_cases as ac
from flight_harness import PLAN_TOL, _compare, agent_states, circle_flight, hdsm  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import _kernel_blocks
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import AssignSetting, agile_params

pytestmark = pytest.mark.gpu

PRM = agile_params(10, max_rows_static=18)


def _same(dev, host, name):
    assert np.array_equal(dev[0], host[0]), (name, "slot_of")
    assert np.array_equal(dev[1], host[1]), (name, "price")
    assert dev[2].tobytes() == host[2].tobytes(), (name, dev[2][:4], host[2][:4])


def test_the_batch_equals_the_host_form_bit_for_bit(hdsm, monkeypatch):  # noqa: F811
    statuses = set()
    for case in ac.cases() + ac.large_cases():
        host, dev = ac.run(case), ac.run(case, device=0)
        _same(dev, host, case[0])
        statuses |= set(host[2]["status"].tolist())
    # the other statuses, the same on both sides: a budget of one iteration, of exactly enough and of one too few; a lowered bid limit
    case = next(c for c in ac.cases() if c[0] == "a partition of 1, 63 and 66")
    need = int(ac.run(case)[2]["iters"].max())
    for max_iters in (1, need, need - 1):
        host, dev = ac.run(case, AssignSetting(max_iters=max_iters)), ac.run(case, AssignSetting(max_iters=max_iters), device=0)
        _same(dev, host, ("budget", max_iters))
        statuses |= set(host[2]["status"].tolist())
    monkeypatch.setenv("HDSM_ASSIGN_BID_LIMIT_LOG2", "30")
    host, dev = ac.run(case), ac.run(case, device=0)
    monkeypatch.delenv("HDSM_ASSIGN_BID_LIMIT_LOG2")
    _same(dev, host, "bid limit")
    statuses |= set(host[2]["status"].tolist())
    assert statuses == {0, 1, 2, 3}, statuses
    # 1025 active agents in one group: refused with nothing touched; 1025 agents, one of them inactive: a full workgroup
    L = hdsm.load()
    big = hdsm.ASSIGN_MAX + 1
    rng = np.random.default_rng(1)
    pos, slots, slot_of = rng.uniform(0, 30, (big, 3)), rng.uniform(0, 30, (big, 3)), np.full(big, -7, np.int32)
    assert L.hdsm_assign_batch(0, None, big, 0, None, pos, None, slots, slot_of, None, None) == hdsm.HDSM_ERR_CAPACITY and (slot_of == -7).all()
    active = np.ones(big, np.uint8)
    active[500] = 0
    _same(hdsm.assign(pos, slots, active=active, device=0), hdsm.assign(pos, slots, active=active), "1025 agents, 1024 active")
    nan_slots = slots.copy()
    nan_slots[3, 0] = np.nan
    assert L.hdsm_assign_batch(0, None, big, 0, None, pos, active, nan_slots, slot_of, None, None) == hdsm.HDSM_ERR_BAD_ARG and (slot_of == -7).all()


def _flight(hdsm, n, groups):  # noqa: F811
    starts, goals = sc.circle_scenario(n, radius=max(4.0, n / 5.0))
    return starts, circle_flight(hdsm, PRM, starts, goals, groups=groups)


@pytest.mark.parametrize("n, groups", [(8, None), (66, [0, 2, 66])])
def test_the_device_loop_assigns_on_its_own_states_and_applies_like_set_goals(hdsm, n, groups):  # noqa: F811
    starts, (sol, loop, dsw) = _flight(hdsm, n, groups)
    for r in range(2):
        _compare(loop, dsw, r)
    states = agent_states(dsw, loop.shard)                       # (the mirror now holds the device's states)
    rng = np.random.default_rng(n)
    slots = sc.grid_formation(n, pitch=2.0, origin=(10.0, 8.0, 1.5))[rng.permutation(n)]
    want = hdsm.assign(states[:, :3], slots, groups=groups)
    assert (want[2]["status"] == 0).all() and not np.array_equal(want[0], np.arange(n))
    due0, goals0 = dsw.mission_due()
    raw0, stats0 = dsw.download_raw(), dsw.path_stats()
    slot_of, stats = dsw.assign(slots, apply=False)
    assert np.array_equal(slot_of, want[0]) and stats.tobytes() == want[2].tobytes()
    due1, goals1 = dsw.mission_due()
    raw1 = dsw.download_raw()
    assert np.array_equal(due0, due1) and np.array_equal(goals0, goals1) and dsw.path_stats() == stats0      # apply = 0: nothing moved
    assert raw0[0].tobytes() == raw1[0].tobytes() and raw0[1].tobytes() == raw1[1].tobytes()
    slot_of, _ = dsw.assign(slots, apply=True)
    m_slot_of, m_stats = loop.shard.assign(slots, apply=True)
    assert np.array_equal(slot_of, want[0]) and np.array_equal(m_slot_of, want[0]) and m_stats.tobytes() == want[2].tobytes()
    due, goals = dsw.mission_due()
    changed = (slots[want[0]] != goals0).any(axis=1)
    assert np.array_equal(goals, slots[want[0]]) and np.array_equal(due != 0, changed | (due0 != 0)) and changed.sum() >= n - 1
    m_due, m_goals = loop.shard.mission_due()
    assert np.array_equal(m_due, due) and np.array_equal(m_goals, goals)
    for r in range(3):                                           # the flight stays with the mirror that was given the same call
        _compare(loop, dsw, 10 + r)
        if r == 0:
            after = dsw.path_stats()
            assert after["planned"] - stats0["planned"] == int((due != 0).sum()) and after["launches"] == stats0["launches"] + 1
    assert not dsw.mission_due()[0].any()
    # under a mission apply = 1 is refused with nothing changed, apply = 0 is not
    dsw.set_mission(sc.mission_setting(1), slots[want[0]][:, None, :])
    before = dsw.mission_due()
    with pytest.raises(hdsm.HdsmError) as e:
        dsw.assign(starts, apply=True)
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "mission" in str(e.value)
    after = dsw.mission_due()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    states = agent_states(dsw, loop.shard)
    assert np.array_equal(dsw.assign(starts, apply=False)[0], hdsm.assign(states[:, :3], starts, groups=groups)[0])
    bad = slots.copy()
    bad[1, 1] = np.inf
    with pytest.raises(hdsm.HdsmError):
        dsw.assign(bad, apply=False)


def test_a_scripted_tail_keeps_minus_one(hdsm):  # noqa: F811
    n, n_script = 8, 2
    starts, (sol, loop, dsw) = _flight(hdsm, n, None)
    dsw.set_script([sc.hold_track(starts[k]) for k in range(n - n_script, n)])
    for r in range(2):
        dsw.round()
    states = agent_states(dsw, loop.shard)
    slots = sc.line_formation(n, pitch=2.0, origin=(10.0, 6.0, 1.5))[::-1].copy()
    active = np.ones(n, np.uint8)
    active[n - n_script:] = 0
    want = hdsm.assign(states[:, :3], slots, active=active)
    goals0 = dsw.mission_due()[1]
    slot_of, stats = dsw.assign(slots, apply=True)
    assert np.array_equal(slot_of, want[0]) and (slot_of[n - n_script:] == -1).all() and stats.tobytes() == want[2].tobytes()
    assert stats["active"][0] == n - n_script and sorted(slot_of[:n - n_script].tolist()) == list(range(n - n_script))
    due, goals = dsw.mission_due()
    assert np.array_equal(goals[:n - n_script], slots[slot_of[:n - n_script]]) and np.array_equal(goals[n - n_script:], goals0[n - n_script:])
    assert not due[n - n_script:].any()                          # (the tail's goals did not change)


def test_fly_formations_line_to_grid_to_line(hdsm):  # noqa: F811
    n = 6
    line = sc.line_formation(n, pitch=2.0, origin=(10.0, 10.0, 1.5))
    grid = sc.grid_formation(n, pitch=2.0, origin=(14.0, 12.0, 1.5), columns=3)
    starts = line + [0.0, 0.0, 0.0]
    sol, loop, dsw = circle_flight(hdsm, PRM, starts, starts + [0.0, 0.5, 0.0])
    rng = np.random.default_rng(2)
    formations = [grid[rng.permutation(n)], line[::-1].copy(), grid]
    summaries, assignments = swarm.fly_formations(dsw, formations, sc.mission_setting(1, arrive_radius=0.3, arrive_speed=0.5), max_rounds=200,
                                                  check_every=4)
    print("fly_formations:", [(s["rounds"], s["done"], s["makespan"]) for s in summaries], [a.tolist() for a in assignments])
    assert len(summaries) == len(assignments) == 3
    for s, a in zip(summaries, assignments):
        assert s["done"] == s["flown"] == n and s["rounds"] < 200, s
        assert sorted(a.tolist()) == list(range(n))
    states = agent_states(dsw, loop.shard)
    assert np.abs(states[:, :3] - grid[assignments[2]]).max() < 0.3 + 1e-9        # everybody stands on the slot it was given


def test_k_assign_uses_no_scratch_and_fits_one_workgroup_of_1024(tmp_path):
    mine = {k: v for k, v in _kernel_blocks(tmp_path).items() if "8k_assignE" in k}
    assert len(mine) == 1, sorted(mine)
    (res,) = mine.values()
    print(res)
    assert res["private_segment_fixed_size"] == 0 and res.get("vgpr_spill_count", 0) == 0 and res.get("sgpr_spill_count", 0) == 0, res
    assert res["vgpr_count"] <= 128 and res["max_flat_workgroup_size"] == 1024, res          # (16 wavefronts on one CU: 128 registers each)
    assert 80 * 1024 <= res["group_segment_fixed_size"] <= 96 * 1024, res                   # coordinates, prices, keys, owners, lists
