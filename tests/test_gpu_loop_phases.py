"""hdsm_dswarm_round, phase by phase: k_corridor (and its packing tail), k_vel_cap -> k_reference -> k_keep_free and k_commit of
csrc/swarm_kernels.hip, each pinned on its own against the independent expectation of tests/loop_cases.py — the oracle's corridor,
a numpy rebuild of the solver inputs handed to a second solver handle, the Python renderings of the velocity cap, KeepOnlyFreeReference,
the read-back / shift and the literal increment walk (tests/refmath.py) — at shapes no other flight uses (loop_cases.SHAPES: both sides
of P * RS = 128, step_plan 2 and 3, use_cvx_new, map radii 0, 7 and 11, n_hor 7 .. 15) and on states edited field by field.
tests/test_loop_phases.py runs the same checks on the host mirror, without a GPU.

Not flown here: a shard with first_id > 0 or padding records. hdsm_dswarm_create takes such a shard only with world_size > 1, and
hdsm_dswarm_round then wants the communicator of that many ranks; one process has one rank. The refusal is tested in place of the
flight (test_a_sharded_device_swarm_refuses_a_round_without_its_communicator), the host mirror flies such a shard in
tests/test_loop_phases.py; the padding branch of k_commit stays unpinned."""
import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
from multi_agent_pkgs_amd import swarm

pytestmark = pytest.mark.gpu

RECORD_TOL = 1e-7   # two runs of the solver stage the neighbour rows in a different order (test_device_resident_loop_follows_the_host_mirror)
KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")


@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    return lib


def device_rounds(hdsm, ctx, loop, rounds, tag):
    """The device loop takes the flight of `loop` over (states, plans) and flies `rounds` rounds; every phase of each is checked."""
    n = ctx.n_rob
    sol, twin_sol = hdsm.Solver(ctx.prm, n, n), hdsm.Solver(ctx.prm, n, n)
    dsw = swarm.DeviceSwarm(loop.shard, sol)
    dsw.upload_plans(loop.plans_all, loop.has_plan)
    fails = 0
    for r in range(rounds):
        pre_plans, pre_has, _, _ = dsw.download(states=True)
        pre = co.export_agents(loop.shard)[0]
        dsw.round()
        plans, has, status, failed = dsw.download(states=True)
        post = co.export_agents(loop.shard)[0]
        # the packing: the inputs rebuilt from the states, solved by a second handle, give the status and the records of the round
        inp = lc.rebuild_inputs(ctx.prm, pre, post)
        twin = twin_sol.replan(*[inp[k] for k in KEYS], pre_plans, pre_has)
        assert (twin["status"] == status).all(), (tag, r, status.tolist(), twin["status"].tolist())
        ok = status != lc.NO_SOLUTION
        if ok.any():
            d = float(np.abs(twin["traj"][ok] - plans[:n][ok]).max())
            assert d < RECORD_TOL, (tag, r, d)
        lc.check_round(ctx, pre, post, pre_plans, pre_has, plans, has, status, solver_out=twin, tol=RECORD_TOL, tag=(tag, r))
        fails += int((status == lc.NO_SOLUTION).sum())
        assert failed == fails, (tag, r, failed, fails)
    dsw.close()
    return ctx.count


def assert_flight_classes(cnt, shape):
    """What 8 rounds of a shape must have shown, counted from the references alone (every shape shows both increments on the host
    mirror within 8 rounds: all are asserted)."""
    assert cnt["made"] - cnt["carried"] > 0 and cnt["carried"] > 0, cnt
    assert cnt["cap_lowered"] > 0, cnt
    assert cnt["inc0"] > 0 and cnt["inc1"] > 0, cnt
    assert cnt["inc_left_out"] * 50 <= cnt["agent_rounds"], cnt
    if shape[5] >= 79:
        assert cnt["stopped_workspace"] > 0 and cnt["made"] > 0, cnt


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_each_phase_of_a_device_round_at_every_shape(hdsm, oracle, shape):
    ctx, loop = lc.make_flight(oracle, shape)
    cnt = device_rounds(hdsm, ctx, loop, lc.ROUNDS, lc.shape_id(shape))
    print("\n%s: %s" % (lc.shape_id(shape), cnt))
    assert_flight_classes(cnt, shape)


CRAFTED = ["startup", "shift-N7", "shift-N10", "shift-N15", "paths", "grid-edges", "far"]


@pytest.mark.parametrize("case", CRAFTED)
def test_crafted_states_through_one_device_round(hdsm, oracle, case):
    """States edited through import_agents before the device takes the flight over (loop_cases.crafted_*), then device rounds
    checked like every other one — one round, or the few the case needs to reach its edge."""
    if case == "startup":
        ctx, loop = lc.crafted_startup_failure(oracle)
        cnt = device_rounds(hdsm, ctx, loop, 1, case)
        assert cnt["failed_without_plan"] > 0 and cnt["solved"] > 0 and cnt["failed_with_plan"] == 0, cnt
    elif case.startswith("shift"):
        shape = {"shift-N7": lc.SHAPES[4], "shift-N10": lc.SHAPES[0], "shift-N15": lc.H15_PLAIN}[case]
        ctx, loop = lc.crafted_shift_edge(oracle, shape)
        cnt = device_rounds(hdsm, ctx, loop, 1, case)
        assert cnt["failed_with_plan"] >= lc.N_AGENTS // 2 and cnt["solved"] > 0, cnt
    elif case == "paths":
        ctx, loop = lc.crafted_paths(oracle)
        cnt = device_rounds(hdsm, ctx, loop, 2, case)
        assert cnt["seg_collision_late"] > 0 and cnt["seg_weak_before"] > 0 and cnt["seg_masked_stronger"] > 0, cnt
    elif case == "grid-edges":
        ctx, loop = lc.crafted_grid_edges(oracle)
        cnt = device_rounds(hdsm, ctx, loop, 2, case)
        assert cnt["kept_free_stops"] > 0 and cnt["ref_past_grid"] > 0 and cnt["near_world_border"] > 0 and cnt["grid_below_ground"] > 0, cnt
    else:
        ctx, loop = lc.make_flight(oracle, lc.SHAPES[0], shift=lc.SHIFT_FAR)
        cnt = device_rounds(hdsm, ctx, loop, lc.ROUNDS, case)
        assert_flight_classes(cnt, lc.SHAPES[0])
    print("\n%s: %s" % (case, cnt))


def test_a_sharded_device_swarm_refuses_a_round_without_its_communicator(hdsm, oracle):
    """15 agents on two ranks: rank 1 holds first_id = 8 and 7 agents, one short of per = 8. hdsm_dswarm_create takes the shard —
    with world_size 2 only — and a round without the communicator of those two ranks is refused before anything is launched: the
    states on the device stay what they were."""
    n_rob, world = 15, 2
    starts, goals = (x[:n_rob] for x in lc.make_scene(0))
    ctx, loop = lc.make_flight(oracle, lc.SHAPES[0], starts=starts, goals=goals, rank=1, world=world, allgather=lambda block: block)
    assert (loop.shard.first_id, loop.shard.n_local) == (8, 7)
    with pytest.raises(hdsm.HdsmError) as e:
        swarm.DeviceSwarm(loop.shard, hdsm.Solver(ctx.prm, 7, n_rob), world_size=1)   # first_id > 0 is no block of one rank
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "first_id" in str(e.value)
    dsw = swarm.DeviceSwarm(loop.shard, hdsm.Solver(ctx.prm, 7, n_rob), world_size=world)
    assert dsw.per == 8
    before = lc.agents_bytes(co.export_agents(loop.shard)[0])
    with pytest.raises(hdsm.HdsmError) as e:
        dsw.round()
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "a sharded swarm needs a communicator" in str(e.value)
    plans, has, _, failed = dsw.download(states=True)
    assert lc.agents_bytes(co.export_agents(loop.shard)[0]) == before and not has.any() and not plans.any() and failed == 0
    assert plans.shape[0] == dsw.per * world
    dsw.close()
