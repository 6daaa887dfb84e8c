"""Local ranks on the MI355X (ABI 1.9): a sharded swarm flown by one process — hdsm_comm_create_local, hdsm_dswarm_round_ranks,
k_gather_local, hdsm_dswarm_download_raw. All ranks share the one device here (the two-device test skips itself on one GPU): the
gather reads the other ranks' send buffers through plain pointers either way, so this is the code a multi-GPU flight runs.

Shapes (n_rob, world), H = 10, 8 rounds of a circle exchange of radius 4 m in free space:
  (16, 2)  even blocks, the control          (10, 3)  per 4, shards 4 / 4 / 2: first_id > 0 and a short last shard (also at H = 15)
  (9, 4)   per 3, an empty fourth rank       (5, 4)   per 2, shards 2 / 2 / 1 / 0       (3, 1)  a group of one
Every round of every flight is checked on the wire, bit for bit (`check_wire`), and against the same swarm flown by hdsm_dswarm_round
on one rank (`check_same_flight`): statuses, failure counts and flags equal, plans within 1e-7 — the tolerance of device loop against
host mirror (tests/test_gpu_configs.py), because the solver's staging order is not bitwise reproducible across launch shapes."""
import ctypes as C

import numpy as np
import pytest

import loop_cases as lc
from flight_harness import circle_flight, device_loop, hdsm  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import assert_no_scratch_no_lds
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8000000000000   # element 0 of a record without a plan; the other rec - 1 elements are +0.0
ROUNDS = 8
PLAN_TOL = 1e-7
SHAPES = [(16, 2), (10, 3), (9, 4), (5, 4), (3, 1)]


def _params(n_hor=10):
    return agile_params(n_hor, max_rows_static=18), swarm.default_swarm_config()


def _slots_with_agent(n_rob, world):
    per = (n_rob + world - 1) // world
    out = np.zeros(world * per, bool)
    for r in range(world):
        first, n_local = swarm.shard_range(n_rob, r, world)
        assert n_local == 0 or first == r * per
        out[r * per:r * per + n_local] = True
    assert out.sum() == n_rob and out[:n_rob].all()     # slot = agent id; everything behind n_rob is padding
    return out


def check_wire(ranks, one_has):
    """Check 1 of one round. one_has: the flags of the same round flown on one rank (which agents have a plan)."""
    world, per, n_rob = ranks.world, ranks.per, ranks.n_rob
    raws = [ranks.download_raw(r) for r in range(world)]
    wire = raws[0][0]
    for r in range(world):
        assert raws[r][0].tobytes() == wire.tobytes(), ("the plans buffers of ranks 0 and %d differ" % r)
    assert wire.tobytes() == np.concatenate([send for _, send in raws]).tobytes(), "the plans buffer is not the concatenation of the send buffers"
    bits = wire.reshape(world * per, -1).view(np.uint64)
    agent = _slots_with_agent(n_rob, world)
    with_plan = agent.copy()
    with_plan[:n_rob] &= one_has[:n_rob] == 1
    # no agent (k >= n_local of a short shard, an empty rank, ids >= n_rob) or no plan yet: the sentinel, exactly
    assert (bits[~with_plan, 0] == SENTINEL).all(), [hex(int(b)) for b in bits[~with_plan, 0]]
    assert (bits[~with_plan, 1:] == 0).all()
    assert not np.isnan(wire.reshape(world * per, -1)[with_plan]).any()
    for r in range(world):
        _, has, _, _ = ranks.dswarms[r].download(states=False)
        assert (has == with_plan).all(), (r, has.tolist(), with_plan.tolist())
    return int((~agent).sum())


def check_same_flight(ranks, one):
    """Check 2 of one round: the ranks together against the one-rank flight."""
    p1, h1, s1, f1 = one.download(states=False)
    status, failed, worst = [], 0, 0.0
    for r in range(ranks.world):
        plans, has, st, nf = ranks.dswarms[r].download(states=False)
        status.append(st)
        failed += nf
        assert (has[:ranks.n_rob] == h1).all(), r
        worst = max(worst, float(np.abs(plans[:ranks.n_rob] - p1).max()))
    status = np.concatenate(status)
    assert (status == s1).all(), (status.tolist(), s1.tolist())
    assert failed == f1, (failed, f1)
    assert worst < PLAN_TOL, worst
    return h1, worst


def _fly(hdsm, n_rob, world, n_hor=10, streams=None, setup=None, scene=None, devices=None, each_round=None):  # noqa: F811
    """ROUNDS rounds of the sharded flight next to the one-rank flight, checks 1 and 2 after every round. Returns both, open."""
    prm, cfg = _params(n_hor)
    starts, goals = sc.circle_scenario(n_rob, radius=4.0) if scene is None else scene
    ranks = swarm.LocalRanks(prm, cfg, n_rob, world, starts=starts, goals=goals, setup=setup, devices=devices)
    sol, loop, one = circle_flight(hdsm, prm, starts, goals, setup=setup)
    worst = pads = 0
    for rnd in range(ROUNDS):
        ranks.round(streams)
        one.round()
        has, w = check_same_flight(ranks, one)
        pads = check_wire(ranks, has)
        worst = max(worst, w)
        if each_round is not None:
            each_round(rnd, ranks, one)
    print("\n(%d, %d) H = %d: %d rounds, %d slots without an agent, max |plans - one rank| %.3e" % (n_rob, world, n_hor, ROUNDS, pads, worst))
    return ranks, (sol, loop, one)


def _close(ranks, one):
    ranks.close()
    one[2].close(), one[0].close()


@pytest.mark.parametrize("n_rob,world", SHAPES, ids=lambda v: str(v))
def test_the_wire_and_the_flight_of_local_ranks(hdsm, n_rob, world):  # noqa: F811
    """Checks 1 and 2 at every shape. The first test that reaches k_commit's padding branch (k >= n: a slot without an agent) and reads
    what it writes raw."""
    ranks, one = _fly(hdsm, n_rob, world)
    per = ranks.per
    assert [d.shard.n_local for d in ranks.dswarms] == [max(0, min(per, n_rob - r * per)) for r in range(world)]
    _close(ranks, one)


def test_h15_where_a_record_is_an_even_number_of_doubles(hdsm):  # noqa: F811
    """(10, 3) at H = 15: rec = 144, every shard starts on a 16-byte boundary of the plans buffer (at H = 10, rec = 99, an odd
    per * rec puts every other shard on an odd double, and k_gather_local moves it with 8-byte accesses)."""
    ranks, one = _fly(hdsm, 10, 3, n_hor=15)
    _close(ranks, one)


def test_streams_three_distinct_and_all_ranks_on_one(hdsm):  # noqa: F811
    """Check 4: (10, 3) once with a stream per rank, once with every rank on one stream (the event waits are then no-ops). One
    flight each."""
    import torch
    three = [torch.cuda.Stream() for _ in range(3)]
    ranks, one = _fly(hdsm, 10, 3, streams=three)
    _close(ranks, one)
    single = torch.cuda.Stream()
    ranks, one = _fly(hdsm, 10, 3, streams=[single] * 3)
    _close(ranks, one)


def test_the_sharded_host_mirror_is_a_second_yardstick(hdsm):  # noqa: F811
    """(10, 3): every rank's block flown as its own host mirror (SwarmLoop with rank / world, the device solver and reference behind
    it), rank by rank in this process the way tests/test_loop_phases.py flies its first_id > 0 shard — the other blocks' records come
    from a one-rank host flight of the same swarm flown before. What each rank's mirror holds after every round equals what the
    device ranks gathered: flags equal, plans within 1e-7."""
    n_rob, world = 10, 3
    prm, cfg = _params()
    starts, goals = sc.circle_scenario(n_rob, radius=4.0)
    per = (n_rob + world - 1) // world
    device_rounds = []

    def keep(rnd, ranks, one):
        plans, has, _, _ = ranks.dswarms[0].download(states=False)
        device_rounds.append((plans[:n_rob], has[:n_rob]))

    ranks, one = _fly(hdsm, n_rob, world, each_round=keep)
    _close(ranks, one)
    sol, whole = device_loop(hdsm, prm, cfg, n_rob, starts=starts, goals=goals)
    records = []
    for _ in range(ROUNDS):
        whole.step()
        records.append((whole.plans_all.copy(), whole.has_plan.copy()))
    rcfg = agile_ref_config()
    for rank in range(world):
        sent = []

        def allgather(block, rank=rank, sent=sent):
            plans, has = records[len(sent)]
            full = np.zeros((world * per,) + plans.shape[1:])
            full[:n_rob] = plans
            full[:n_rob][has == 0, 0, 0] = np.nan
            full[n_rob:, 0, 0] = np.nan
            assert block.shape[0] == per
            full[rank * per:(rank + 1) * per] = block
            sent.append(block.copy())
            return full

        def solve(inp, plans, has):
            return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

        def ref_dev(ids, path, n_path, plans, has, vel_cap=None):
            full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
            return full, pv

        sol.reset_warm_start()
        loop = swarm.SwarmLoop(prm, cfg, n_rob, rank=rank, world=world, solve=solve, allgather=allgather, reference=ref_dev, starts=starts, goals=goals)
        assert (loop.shard.first_id, loop.shard.n_local) == swarm.shard_range(n_rob, rank, world)
        for rnd in range(ROUNDS):
            loop.step()
            plans, has = device_rounds[rnd]
            assert (loop.has_plan == has).all(), (rank, rnd)
            assert np.abs(loop.plans_all - plans).max() < PLAN_TOL, (rank, rnd, float(np.abs(loop.plans_all - plans).max()))
            n_local = loop.shard.n_local   # the block it sent: its records, and the sentinel in the padding slots of the short shard
            pad = sent[rnd][n_local:].reshape(per - n_local, (prm.n_hor + 1) * 9)
            assert np.isnan(pad[:, 0]).all() and not pad[:, 1:].any(), (rank, rnd)
    sol.close()


INT_FIELDS = ("rounds", "positions", "close_rounds", "occupied", "unknown", "crossed", "pot_sum")
SEP_FIELDS = ("sep_partner", "sep_substep", "sep_round")


def test_the_audit_across_ranks_on_the_pillar_flight(hdsm):  # noqa: F811
    """Check 3, first part. (10, 3) through the 120 x 120 x 30 pillar world of tests/loop_cases.py, path period 1, audit on: the
    per-agent flight reports of the ranks, concatenated, against the one-rank flight's — every integer field equal, sep2_min, dist
    and the speeds to 1e-9 relative. Where the two flights name different partners (or sub-steps, or rounds) for an agent's minimum
    — a tie, decided by the last bits of plans that agree to 1e-7 — only sep2_min is compared for that agent, and the test says so."""
    grid, worigin = lc.make_world()
    scene = tuple(x[:10] for x in lc.make_scene(0))

    def setup(shard, rank):
        shard.set_world(grid, worigin)
        shard.set_path_period(1)
        shard.set_audit(True, 1.0)

    ranks, one = _fly(hdsm, 10, 3, setup=setup, scene=scene)
    got = np.concatenate([d.flight_report() for d in ranks.dswarms])
    want = one[2].flight_report()
    assert got.shape == want.shape == (10,) and want["rounds"].max() == ROUNDS
    for name in INT_FIELDS:
        assert np.array_equal(got[name], want[name]), (name, got[name].tolist(), want[name].tolist())
    ties = np.zeros(10, bool)
    for name in SEP_FIELDS:
        ties |= got[name] != want[name]
    if ties.any():
        print("agents whose minimum is a tie between two partners / sub-steps / rounds (sep2_min alone compared):", np.nonzero(ties)[0].tolist())
    for name in ("sep2_min", "dist", "speed_sum", "speed_max"):
        rel = np.abs(got[name] - want[name]) / np.maximum(np.abs(want[name]), 1e-300)
        assert (rel <= 1e-9).all(), (name, rel.tolist())
    assert (want["sep_partner"] >= 0).all()
    stats = [d.path_stats() for d in ranks.dswarms]
    assert sum(s["planned"] for s in stats) == one[2].path_stats()["planned"] == 10 * ROUNDS      # the path step ran on every rank
    _close(ranks, one)


def _fold_groups(reports):
    """The group reports of the ranks put together as k_group_report would over all agents: sums, the maximum of `rounds`, the
    smallest sep2_min with ties to the lower agent id."""
    out = reports[0].copy()
    for rep in reports[1:]:
        assert np.array_equal(rep["first"], out["first"]) and np.array_equal(rep["count"], out["count"])
        for name in ("n_local", "no_solution_last", "failed_total", "positions", "close_rounds", "occupied", "unknown", "crossed", "pot_sum"):
            out[name] += rep[name]
        out["rounds"] = np.maximum(out["rounds"], rep["rounds"])
        for g in range(out.size):
            a, b = out[g], rep[g]
            if b["sep_agent"] >= 0 and (a["sep_agent"] < 0 or (b["sep2_min"], b["sep_agent"]) < (a["sep2_min"], a["sep_agent"])):
                for name in ("sep2_min", "sep_agent", "sep_partner", "sep_substep", "sep_round"):
                    out[name][g] = b[name]
    return out


def test_groups_across_ranks(hdsm):  # noqa: F811
    """Check 3, second part. (16, 2) with the groups [0, 5, 11, 16]: the middle group straddles the rank boundary at agent 8. The
    flight is the one-rank grouped flight's (checks 1 and 2 every round), and hdsm_dswarm_group_report folded over the ranks equals
    the one-rank report in the integer fields (the audit is on, so that they hold something)."""
    groups = [0, 5, 11, 16]

    def setup(shard, rank):
        shard.set_groups(groups)
        shard.set_audit(True, 1.0)

    ranks, one = _fly(hdsm, 16, 2, setup=setup)
    per_rank = [d.group_report() for d in ranks.dswarms]
    assert [r["n_local"].tolist() for r in per_rank] == [[5, 3, 0], [0, 3, 5]]
    got, want = _fold_groups(per_rank), one[2].group_report()
    for name in ("first", "count", "n_local", "no_solution_last", "failed_total", "rounds", "positions", "close_rounds", "occupied", "unknown",
                 "crossed", "pot_sum", "sep_agent"):
        assert np.array_equal(got[name], want[name]), (name, got[name].tolist(), want[name].tolist())
    assert want["rounds"].tolist() == [ROUNDS] * 3 and (want["sep_agent"] >= 0).all()
    assert (np.abs(got["sep2_min"] - want["sep2_min"]) <= 1e-9 * want["sep2_min"]).all()
    # every agent's closest partner is one of its own group, on either side of the rank boundary
    rep = np.concatenate([d.flight_report() for d in ranks.dswarms])
    for lo, hi in zip(groups[:-1], groups[1:]):
        p = rep["sep_partner"][lo:hi]
        assert ((p >= lo) & (p < hi)).all(), (lo, p.tolist())
    _close(ranks, one)


def _arr(items):
    return (C.c_void_p * len(items))(*items)


def test_refusals_launch_nothing(hdsm):  # noqa: F811
    """Check 5. Every refusal returns HDSM_ERR_BAD_ARG before anything is launched or booked: refusals are made before the first
    round and between the rounds of a (10, 3) flight, and the flight is still the one-rank flight, round for round."""
    L = hdsm.load()
    prm, cfg = _params()
    starts, goals = sc.circle_scenario(10, radius=4.0)
    ranks = swarm.LocalRanks(prm, cfg, 10, 3, starts=starts, goals=goals)
    sol, loop, one = circle_flight(hdsm, prm, starts, goals)
    d = [x.h.value for x in ranks.dswarms]
    c = ranks.comms

    def refused(world, dsw, comms, text):
        rc = L.hdsm_dswarm_round_ranks(world, _arr(dsw), _arr(comms), None)
        assert rc == hdsm.HDSM_ERR_BAD_ARG and text in L.hdsm_dswarm_last_error().decode(), (rc, L.hdsm_dswarm_last_error())

    def refusals():
        refused(2, d[:2], c[:2], "the local group has 3 ranks")                       # a world that does not match the group
        refused(3, [d[0], d[1], d[1]], [c[0], c[1], c[1]], "every rank once")          # a rank given twice
        refused(3, [d[0], d[1], d[1]], c, "given again")                               # ... its dswarm alone
        refused(3, [d[1], d[0], d[2]], c, "do not match the shard")                    # a dswarm cut for another rank's block
        refused(3, d, [c[0], c[1], None], "null")
        assert L.hdsm_dswarm_round(d[0], c[0], None) == hdsm.HDSM_ERR_BAD_ARG           # a local communicator where an RCCL one belongs
        assert "hdsm_dswarm_round_ranks" in L.hdsm_dswarm_last_error().decode()
        assert L.hdsm_exchange_device(c[0], ranks.per, None, None, None, None) == hdsm.HDSM_ERR_BAD_ARG
        assert "hdsm_dswarm_round_ranks" in L.hdsm_last_error().decode()
        assert L.hdsm_dswarm_round(d[1], None, None) == hdsm.HDSM_ERR_BAD_ARG           # (as before: a sharded swarm needs a communicator)

    refusals()
    for rnd in range(3):
        ranks.round()
        one.round()
        has, _ = check_same_flight(ranks, one)
        check_wire(ranks, has)
        refusals()
    r, w = C.c_int32(-1), C.c_int32(-1)
    assert L.hdsm_comm_info(c[2], C.byref(r), C.byref(w)) == 0 and (r.value, w.value) == (2, 3)
    ranks.close(), one.close(), sol.close()


def test_an_rccl_communicator_is_no_local_rank(hdsm):  # noqa: F811
    """Check 5, last item: an RCCL communicator of one rank given to hdsm_dswarm_round_ranks. Skipped where RCCL cannot make one."""
    L = hdsm.load()
    prm, cfg = _params()
    starts, goals = sc.circle_scenario(3, radius=4.0)
    ranks = swarm.LocalRanks(prm, cfg, 3, 1, starts=starts, goals=goals)
    try:
        rccl = hdsm.Comm(ranks.solvers[0], hdsm.comm_unique_id(), 0, 1)
    except hdsm.HdsmError as e:
        ranks.close()
        pytest.skip("no RCCL communicator on this machine: %s" % e)
    rc = L.hdsm_dswarm_round_ranks(1, _arr([ranks.dswarms[0].h.value]), _arr([rccl.h.value]), None)
    assert rc == hdsm.HDSM_ERR_BAD_ARG and "not a local one" in L.hdsm_dswarm_last_error().decode()
    ranks.round()                                       # ... and the group of one goes on: through the send buffer
    plans, send = ranks.download_raw(0)
    assert plans.tobytes() == send.tobytes() and not np.isnan(plans).any()
    rccl.close()
    ranks.close()


def test_one_rank_per_device(hdsm):  # noqa: F811
    """Check 6: (10, 2), rank r on device r, the send buffers read across devices through peer access. Needs two GPUs."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: the peer path of k_gather_local cannot run here")
    ranks, one = _fly(hdsm, 10, 2, devices=[0, 1])
    _close(ranks, one)


def test_download_raw_on_a_plain_single_rank(hdsm):  # noqa: F811
    """Without a communicator a single rank publishes straight into the plans buffer: the send buffer stays unused and comes back as
    zeros; either pointer may be NULL."""
    prm, cfg = _params()
    starts, goals = sc.circle_scenario(3, radius=4.0)
    sol, loop, one = circle_flight(hdsm, prm, starts, goals)
    one.round()
    plans, send = np.full((3, 11, 9), 7.0), np.full((3, 11, 9), 7.0)
    hdsm.call("hdsm_dswarm_download_raw", one.h, plans, send)
    assert not send.any() and np.array_equal(plans, one.download(states=False)[0]) and plans[:, 1, :3].any()
    hdsm.call("hdsm_dswarm_download_raw", one.h, None, None)
    hdsm.call("hdsm_dswarm_download_raw", one.h, None, send)
    one.close(), sol.close()


@pytest.mark.parametrize("src_odd,dst_odd", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=["aligned", "both-odd", "dst-odd", "src-odd"])
def test_gather_kernel_at_every_alignment(hdsm, src_odd, dst_odd):  # noqa: F811
    """k_gather_local alone (hdsm_internal_gather_local_launch) on buffers that start on an even or an odd double: 16-byte accesses
    where source and destination agree modulo 16 bytes — with a ragged head when both are odd — and 8-byte accesses where they do
    not. world 3, per 3, rec 99 (per * rec odd: the shards of the plans buffer alternate between the two boundaries by themselves),
    and rec 144. The bytes around the destination stay as they were."""
    import torch
    L = hdsm.load()
    L.hdsm_internal_gather_local_launch.restype = C.c_int
    L.hdsm_internal_gather_local_launch.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(3)
    for world, per, rec in ((3, 3, 99), (2, 5, 144), (4, 1, 99)):
        n = per * rec
        host = rng.standard_normal((world, n))
        host.reshape(world, per, rec)[rng.random((world, per)) < 0.4, 0] = np.nan
        host.reshape(world, per, rec)[0, 0, 0] = np.nan
        send = [torch.zeros(n + 2, dtype=torch.float64, device="cuda") for _ in range(world)]
        for r in range(world):
            send[r][src_odd:src_odd + n] = torch.from_numpy(host[r]).cuda()
        table = torch.tensor([s.data_ptr() + 8 * src_odd for s in send], dtype=torch.int64, device="cuda")
        lo = 2 + dst_odd             # (a tensor starts on a 256-byte boundary)
        assert all(s.data_ptr() % 16 == 0 for s in send)
        plans = torch.full((world * n + 6,), -5.0, dtype=torch.float64, device="cuda")
        has = torch.full((world * per + 2,), 9, dtype=torch.uint8, device="cuda")
        assert plans.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        rc = L.hdsm_internal_gather_local_launch(world, per, rec, table.data_ptr(), plans.data_ptr() + 8 * lo, has.data_ptr() + 1, None)
        assert rc == 0, L.hdsm_last_error()
        torch.cuda.synchronize()
        got, flags = plans.cpu().numpy(), has.cpu().numpy()
        assert got[lo:lo + world * n].tobytes() == host.tobytes(), (world, per, rec)
        assert (got[:lo] == -5.0).all() and (got[lo + world * n:] == -5.0).all()
        assert flags[0] == 9 and flags[-1] == 9
        assert (flags[1:-1] == ~np.isnan(host.reshape(world * per, rec)[:, 0])).all()


def test_gather_kernel_uses_no_scratch_and_no_lds(tmp_path):
    """Check 7: k_gather_local as built into the library — private segment 0, no spills, group segment 0."""
    assert_no_scratch_no_lds(tmp_path, "k_gather_local")
