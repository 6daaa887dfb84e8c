"""Every phase of a round of the closed loop, pinned on its own against something independent (tests/loop_cases.py), on the HOST
MIRROR (csrc/swarm_host.cpp, the per-agent code of csrc/swarm_core.h) at the shapes of loop_cases.SHAPES and on the crafted states —
what the device test (tests/test_gpu_loop_phases.py) flies: this file validates the renderings of tests/refmath.py and the shared
source there first. The loop is SwarmLoop with the oracle as the solver and the oracle's orc_reference as the reference."""
import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
from multi_agent_pkgs_amd import swarm


def assert_flight_classes(cnt, shape):
    """What 8 rounds of a shape must have shown, counted from the references alone."""
    assert cnt["made"] - cnt["carried"] > 0 and cnt["carried"] > 0, cnt   # polyhedra were carried over AND newly made
    assert cnt["cap_lowered"] > 0, cnt
    assert cnt["inc0"] > 0 and cnt["inc1"] > 0, cnt                       # (every shape shows both within 8 rounds)
    assert cnt["inc_left_out"] * 50 <= cnt["agent_rounds"], cnt
    if shape[5] >= 79:   # wave_map_radius = 0: polyhedra beyond the fixed workspace are refused on both sides — and not all are
        assert cnt["stopped_workspace"] > 0 and cnt["made"] > 0, cnt


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_each_phase_of_a_host_round_at_every_shape(oracle, shape):
    ctx, loop = lc.make_flight(oracle, shape)
    cnt = lc.host_rounds(ctx, loop, lc.ROUNDS, lc.shape_id(shape))
    print("\n%s: %s" % (lc.shape_id(shape), cnt))
    assert_flight_classes(cnt, shape)


def test_startup_failure_on_the_host(oracle):
    ctx, loop = lc.crafted_startup_failure(oracle)
    cnt = lc.host_rounds(ctx, loop, 1, "startup")
    print("\nstartup failure: %s" % cnt)
    assert cnt["failed_without_plan"] > 0 and cnt["solved"] > 0 and cnt["failed_with_plan"] == 0, cnt


@pytest.mark.parametrize("shape", [lc.SHAPES[4], lc.SHAPES[0], lc.H15_PLAIN], ids=lc.shape_id)
def test_shift_of_a_distinct_plan_on_the_host(oracle, shape):
    ctx, loop = lc.crafted_shift_edge(oracle, shape)
    cnt = lc.host_rounds(ctx, loop, 1, "shift")
    print("\nshift edge %s: %s" % (lc.shape_id(shape), cnt))
    assert cnt["failed_with_plan"] >= lc.N_AGENTS // 2 and cnt["solved"] > 0, cnt


def test_path_edges_on_the_host(oracle):
    ctx, loop = lc.crafted_paths(oracle)
    cnt = lc.host_rounds(ctx, loop, 2, "paths")
    print("\npath edges: %s" % cnt)
    assert cnt["seg_collision_late"] > 0 and cnt["seg_weak_before"] > 0 and cnt["seg_masked_stronger"] > 0, cnt


def test_grid_edges_on_the_host(oracle):
    ctx, loop = lc.crafted_grid_edges(oracle)
    cnt = lc.host_rounds(ctx, loop, 2, "edges")
    print("\ngrid edges: %s" % cnt)
    assert cnt["kept_free_stops"] > 0 and cnt["ref_past_grid"] > 0 and cnt["near_world_border"] > 0 and cnt["grid_below_ground"] > 0, cnt


def test_far_from_the_origin_on_the_host(oracle):
    """The swarm of the first shape 1e4 m away in x, the world with it: the guard of the increment check and the truncations
    (int)((p - origin) / voxel) depend on the magnitude of the coordinates."""
    ctx, loop = lc.make_flight(oracle, lc.SHAPES[0], shift=lc.SHIFT_FAR)
    cnt = lc.host_rounds(ctx, loop, lc.ROUNDS, "far")
    print("\nfar: %s" % cnt)
    assert_flight_classes(cnt, lc.SHAPES[0])


def test_a_short_trailing_shard_on_the_host(oracle):
    """first_id > 0 and a shard shorter than per: 15 agents on two ranks are blocks of 8 and 7. Rank 1 flies its 7 agents as its own
    SwarmLoop; the other block's records come from a single-rank flight of the same swarm flown before (the oracle is deterministic:
    both flights are the same flight). Every round of rank 1 is checked like any other — the expectation indexes the records by
    agent id, first_id + k — and the block it sends carries the sentinel in its padding slot and in the slots of agents without a
    plan. (The device loop cannot fly this shard in one process: tests/test_gpu_loop_phases.py tests its refusal.)"""
    shape, n_rob, per = lc.SHAPES[0], 15, 8
    starts, goals = (x[:n_rob] for x in lc.make_scene(0))
    _, whole = lc.make_flight(oracle, shape, starts=starts, goals=goals)
    records = []
    for _ in range(lc.ROUNDS):
        whole.step()
        records.append((whole.plans_all.copy(), whole.has_plan.copy()))
    sent = []

    def allgather(block):
        blk0, has0 = records[len(sent)][0][:per].copy(), records[len(sent)][1][:per]
        blk0[has0 == 0, 0, 0] = np.nan
        sent.append(block.copy())
        return np.concatenate([blk0, block])

    ctx, loop = lc.make_flight(oracle, shape, starts=starts, goals=goals, rank=1, world=2, allgather=allgather)
    assert (ctx.first_id, loop.shard.first_id, loop.shard.n_local) == (per, per, n_rob - per)
    for r in range(lc.ROUNDS):
        cnt = lc.host_rounds(ctx, loop, 1, ("rank1", r))
        block, (plans, has) = sent[r], records[r]
        assert block.shape[0] == per and np.isnan(block[per - 1, 0, 0]) and not block[per - 1].reshape(-1)[1:].any()   # the padding slot
        for k in range(n_rob - per):   # a local slot: the record, or the sentinel while the agent has no plan
            if loop.has_plan[per + k]:
                assert np.array_equal(block[k], loop.plans_all[per + k])
            else:
                assert np.isnan(block[k, 0, 0]) and not block[k].reshape(-1)[1:].any()
        assert loop.plans_all.shape[0] == n_rob and np.array_equal(loop.has_plan, has)
        assert np.array_equal(loop.plans_all[:per], plans[:per]) and np.array_equal(loop.plans_all[per:], plans[per:])
    print("\nrank 1 of 2: %s" % cnt)
    assert_flight_classes(cnt, shape)


def test_agent_state_mirror_survives_a_round_trip(oracle):
    """tests/corridor_oracle.py mirrors hdsm_sw::AgentS field by field with MAXH, MAXP, RSMAX and PATH_PTS written out; the library
    reports no sizeof, so: export, import, export again — byte-identical, on states that a flight has filled up to the last field
    (a mirror of another size would cut the array short or shift the second agent)."""
    ctx, loop = lc.make_flight(oracle, lc.SHAPES[0])
    for _ in range(2):
        loop.step()
    first = co.export_agents(loop.shard)[0]
    assert [first[a].id for a in range(lc.N_AGENTS)] == list(range(lc.N_AGENTS))          # the stride is right: every id where it belongs
    assert all(first[a].n_ref == ctx.prm.n_hor + 1 and first[a].path_vel > 0 for a in range(lc.N_AGENTS))   # ... up to the last field
    twin = swarm.SwarmShard(ctx.prm, ctx.cfg, lc.N_AGENTS, 0, np.zeros((lc.N_AGENTS, 3)), np.ones((lc.N_AGENTS, 3)))
    lc.import_agents(twin, first)
    second = co.export_agents(twin)[0]
    assert lc.agents_bytes(first) == lc.agents_bytes(second)
    pos = twin.state()[0]
    assert np.array_equal(pos, np.array([lc.arr(first[a].state_curr, 9)[:3] for a in range(lc.N_AGENTS)]))
