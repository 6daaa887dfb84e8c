"""Shapes, world, state round trips and the independent expectation of ONE ROUND of the closed loop — shared by
tests/test_loop_phases.py (the host mirror, CPU) and tests/test_gpu_loop_phases.py (hdsm_dswarm_round). TEST INFRASTRUCTURE, no tests.

A round takes the planner states of the agents (hdsm_sw::AgentS, csrc/swarm_core.h) and the plans everybody published, and leaves
new states and new records. `check_round` looks at the states before and after and pins every phase on its own against something
that shares no source with the loop:

  corridor    oracle/hdsm_oracle.c: orc_safe_corridor on the state before (tests/corridor_oracle.py), bit for bit
  packing     the solver inputs rebuilt here in numpy from the states, with the layouts of include/hdsm.h (`rebuild_inputs`)
  reference   the polyline of a twin host mirror, the velocity cap and KeepOnlyFreeReference of tests/refmath.py (Python renderings of
              AC:1695-1767 and AC:1665-1693, 1527-1547), the oracle's orc_reference between them
  commit      the read-back / shift of AC:955-1019 and the literal walk of CheckReferenceTrajIncrement / GetPathProgress as rendered in
              tests/refmath.py, from the state before and the round's own status
(AC = multi_agent_planner/src/agent_class.cpp of the reference.)"""
import ctypes as C
import math

import numpy as np

import corridor_oracle as co
import refmath
from multi_agent_pkgs_amd import lib as hdsm
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

NO_SOLUTION = 2   # HDSM_NO_SOLUTION
N_AGENTS = 16
ROUNDS = 8

# (n_hor, poly_hor, max_rows_static, step_plan, use_cvx_new, n_it_decomp, thresh_dist): the smallest shapes that reach each branch of
# the loop's kernels (csrc/swarm_kernels.hip). No shape was refused by hdsm_swarm_create / hdsm_dswarm_create: none is replaced.
SHAPES = [
    (10, 4, 18, 1, 0, 42, 1.0),    # the shape every other loop test flies: the control
    (10, 4, 32, 1, 1, 42, 1.0),    # P * RS = 128: last shape of the cooperative corridor, two rows per lane exactly, shape-aware variant
    (10, 5, 32, 2, 0, 30, 1.0),    # P * RS = 160: first shape of the plain corridor on lane 0, step_plan = 2, map radius 7
    (15, 8, 32, 3, 1, 54, 0.05),   # every capacity at its maximum, N * 9 = 135 (third slot per lane of the shift), tight thresh_dist
    (7, 2, 18, 1, 0, 80, 1.0),     # shortest horizon, wave_map_radius = 0 (the plain decomposition out of the LDS slab)
    (12, 7, 18, 1, 0, 42, 0.3),    # P * RS = 126, more than 4 polyhedra on the cooperative corridor
]


H15_PLAIN = (15, 4, 18, 1, 0, 42, 1.0)   # H = 15 with the corridor of the control: what the crafted states at n_hor 15 fly


def shape_id(shape):
    return "N%d-P%d-RS%d-step%d-new%d-it%d-th%g" % shape


def shape_params(shape):
    n_hor, poly_hor, rs, step_plan, use_new, n_it, thresh = shape
    prm = agile_params(n_hor, poly_hor=poly_hor, max_rows_static=rs)
    cfg = swarm.default_swarm_config()
    cfg.step_plan, cfg.use_cvx_new, cfg.n_it_decomp, cfg.thresh_dist = step_plan, use_new, n_it, thresh
    return prm, cfg


WORLD_ORIGIN = np.array([-3.0, -6.0, -0.9])
PILLARS = [(30, 40), (34, 52), (41, 45), (47, 58), (52, 38), (58, 50), (64, 43), (70, 55), (76, 47), (45, 70), (60, 30), (83, 40)]


def make_world(shift=(0.0, 0.0, 0.0)):
    """120 x 120 x 30 voxels of 0.3 m: a dozen full-height pillars, inflated (100), a halo of 60 within 0.6 m of them and of 25
    within 1.2 m (a crude potential field, built like the worlds of test_voxel_velocity_cap_and_keep_only_free_follow_the_reference_
    statements). Returns (world int8 [nz][ny][nx], origin)."""
    raw = np.zeros((30, 120, 120), np.int8)
    for i, j in PILLARS:
        raw[:, j, i] = 100
    occ = sc.inflate(raw)
    near = sc.inflate(occ, inflation_dist=0.6)
    far = sc.inflate(occ, inflation_dist=1.2)
    world = np.where(occ >= 100, 100, np.where(near >= 100, 60, np.where(far >= 100, 25, 0))).astype(np.int8)
    return world, WORLD_ORIGIN + np.asarray(shift, dtype=np.float64)


def make_scene(seed=0, shift=(0.0, 0.0, 0.0)):
    """16 agents in two facing rows on either side of the pillars, each flying to a place in the other row."""
    rng = np.random.default_rng(seed)
    y = 3.0 + 1.7 * np.arange(8) + rng.uniform(-0.2, 0.2, 8)
    left = np.stack([np.full(8, 4.0) + rng.uniform(-0.5, 0.5, 8), y, 1.5 + rng.uniform(-0.3, 0.3, 8)], axis=1)
    right = np.stack([np.full(8, 24.0) + rng.uniform(-0.5, 0.5, 8), y[::-1] + 0.4, 1.5 + rng.uniform(-0.3, 0.3, 8)], axis=1)
    starts = np.concatenate([left, right])
    goals = np.concatenate([right[rng.permutation(8)], left[rng.permutation(8)]]) + [0.0, 0.3, 0.0]
    return starts + np.asarray(shift), goals + np.asarray(shift)


def open_scene(seed=1):
    """16 agents in the strip of the world that holds no pillar (x in 25 .. 32), two columns swapping sides: the corridors are the
    boxes of free space and the solves are easy — for the cases that are about something else than the corridor."""
    rng = np.random.default_rng(seed)
    y = 4.0 + 1.6 * np.arange(8)
    left = np.stack([np.full(8, 25.5), y, 1.5 + rng.uniform(-0.3, 0.3, 8)], axis=1)
    right = np.stack([np.full(8, 31.5), y + 0.4, 1.5 + rng.uniform(-0.3, 0.3, 8)], axis=1)
    return np.concatenate([left, right]), np.concatenate([right[rng.permutation(8)], left[rng.permutation(8)]]) + [0.0, 0.3, 0.0]


def import_agents(shard, buf):
    """The inverse of corridor_oracle.export_agents (hdsm_swarm_import_state): the states `buf` (an AgentS array of n_local
    entries) become the host mirror's."""
    L = hdsm.load()
    L.hdsm_swarm_import_state.restype = C.c_int
    L.hdsm_swarm_import_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    rc = L.hdsm_swarm_import_state(shard.h, C.cast(buf, C.c_void_p), shard.n_local)
    assert rc == 0, rc


def agents_bytes(buf):
    return bytes(memoryview(buf).cast("B"))


def arr(field, *shape):
    """A ctypes array field of an AgentS as a numpy array (a copy)."""
    return np.frombuffer(bytes(memoryview(field).cast("B")), dtype=np.float64).reshape(shape).copy()


class Round:
    """What check_round needs of the flight: configuration, world, and the counters of what the rounds showed."""

    def __init__(self, orc, prm, cfg, world, worigin, n_rob, first_id=0):
        self.orc, self.prm, self.cfg, self.world, self.worigin = orc, prm, cfg, world, np.asarray(worigin, dtype=np.float64)
        self.n_rob, self.first_id = n_rob, first_id
        self.rcfg = agile_ref_config(path_vel_min=cfg.path_vel_min, path_vel_max=cfg.path_vel_max, sens_dist=cfg.sens_dist,
                                     sens_pot=cfg.sens_pot, sens_other_agents=cfg.sens_other_agents, path_vel_dec=cfg.path_vel_dec)
        self.twin = None
        self.count = dict(agent_rounds=0, carried=0, made=0, corridor_stopped=0, cap_lowered=0, kept_free_stops=0, inc0=0, inc1=0,
                          inc_left_out=0, solved=0, failed_with_plan=0, failed_without_plan=0,
                          seg_collision_late=0, seg_masked_stronger=0, seg_weak_before=0,
                          stopped_seed_outside=0, stopped_rows=0, stopped_workspace=0, ref_past_grid=0, near_world_border=0,
                          grid_below_ground=0)

    def dims(self):
        vs = self.cfg.voxel_size
        return tuple(int(math.floor(self.cfg.grid_range[k] / vs)) for k in range(3))


def rebuild_inputs(prm, pre, post):
    """agent_id, state, ref, n_poly, n_rows, A, b of include/hdsm.h from the agent states: state_curr of the state BEFORE the round,
    the polyhedra and traj_ref[:N] of the state after it; rows past `rows` and polyhedra past n_poly are zero."""
    n, N, P, RS = len(post), prm.n_hor, prm.poly_hor, prm.max_rows_static
    inp = dict(agent_id=np.zeros(n, np.int32), state=np.zeros((n, 9)), ref=np.zeros((n, N, 6)), n_poly=np.zeros(n, np.int32),
               n_rows=np.zeros((n, P), np.int32), A=np.zeros((n, P, RS, 3)), b=np.zeros((n, P, RS)))
    for a in range(n):
        inp["agent_id"][a] = post[a].id
        inp["state"][a] = arr(pre[a].state_curr, 9)
        inp["ref"][a] = arr(post[a].traj_ref, co.MAXH + 1, 6)[:N]
        inp["n_poly"][a] = post[a].n_poly
        for j in range(post[a].n_poly):
            r = post[a].polys[j].rows
            inp["n_rows"][a, j] = r
            inp["A"][a, j, :r] = arr(post[a].polys[j].A, co.RSMAX, 3)[:r]
            inp["b"][a, j, :r] = arr(post[a].polys[j].b, co.RSMAX)[:r]
    return inp


def _twin(ctx, pre):
    """A host mirror of its own that takes the states `pre` over (for the polyline of this round's reference)."""
    n = len(pre)
    if ctx.twin is None or ctx.twin.n_local != n:
        ctx.twin = swarm.SwarmShard(ctx.prm, ctx.cfg, ctx.n_rob, ctx.first_id, np.zeros((n, 3)), np.ones((n, 3)))
        ctx.twin.set_world(ctx.world, ctx.worigin)
    import_agents(ctx.twin, pre)
    ctx.twin.prepare_corridor()
    return ctx.twin.reference_inputs(pmax=co.PATH_PTS + 2)


def increment_guard(point):
    """The guard of k_commit's closed form: decisions closer than this to d0 or thresh_dist are walked literally there, and left
    out of the exact compare here."""
    return 1e-9 * max(1.0, 0.01 * max(abs(float(c)) for c in point))


def check_corridor(ctx, pre, post, tag=""):
    made = carried = 0
    for a in range(len(pre)):
        del co.REFUSALS[:]
        rc, want = co.oracle_corridor(ctx.orc.lib(), ctx.prm, ctx.cfg, ctx.world, ctx.worigin, pre[a])
        got = co.product_corridor(post[a])
        # a seed outside the grid (-1), a polyhedron beyond the row capacity or the fixed workspace (-4): both sides stop with the
        # same code, at the same polyhedron — what was kept and made before the stop is compared like a finished corridor
        assert rc == post[a].corridor_rc, (tag, a, rc, post[a].corridor_rc)
        assert co.same_corridor(got, want), (tag, a, rc, [g[0] for g in got], [w[0] for w in want])
        if rc != 0:
            assert len(co.REFUSALS) == 1, (tag, a, co.REFUSALS)
            ctx.count["corridor_stopped"] += 1
            ctx.count["stopped_" + co.REFUSALS[0]] += 1
        old = co.product_corridor(pre[a])
        carried += sum(1 for g in got if any(np.array_equal(g[3], h[3]) for h in old))
        made += len(got)
    ctx.count["carried"] += carried
    ctx.count["made"] += made


def expected_reference(ctx, pre, pre_plans, pre_has):
    """(ref_full [n][N+1][6], path_vel [n], stop [n], caps [n], segs per agent) of this round from the states before it."""
    n, N = len(pre), ctx.prm.n_hor
    path, n_path = _twin(ctx, pre)
    vs, dim = ctx.cfg.voxel_size, ctx.dims()
    caps, segs, origins, vals = np.zeros(n), [], [], []
    for a in range(n):
        go = refmath.local_grid_origin(arr(pre[a].state_curr, 9)[:3], ctx.cfg.grid_range, vs)
        val = refmath.window_value(ctx.world, ctx.worigin, go, dim, ctx.cfg.grid_z_min, vs)
        caps[a], s = refmath.path_velocity_cap(val, dim, go, vs, path[a, :n_path[a]], ctx.cfg.path_vel_min, ctx.cfg.path_vel_max,
                                               ctx.cfg.sens_pot, ctx.cfg.sens_dist)
        segs.append(s), origins.append(go), vals.append(val)
        # where the agent stands: within two voxels of the world's border in x or y; 8 or more of the grid's levels below the ground
        pos, wmax = arr(pre[a].state_curr, 9)[:3], ctx.worigin + np.array(ctx.world.shape[::-1]) * vs
        ctx.count["near_world_border"] += int(any(0 <= (pos[k] - ctx.worigin[k]) / vs < 2 or 0 <= (wmax[k] - pos[k]) / vs < 2 for k in (0, 1)))
        ctx.count["grid_below_ground"] += int(math.ceil((ctx.cfg.grid_z_min - go[2]) / vs - 1e-9) >= 8)
    ids = np.array([pre[a].id for a in range(n)], np.int32)
    full, _, pv = ctx.orc.reference(ctx.prm, ctx.rcfg, ids, path, n_path, pre_plans, pre_has, vel_cap=caps)
    want, stop = np.zeros((n, N + 1, 6)), np.zeros(n, np.int32)
    for a in range(n):
        pts, stop[a] = refmath.keep_only_free(full[a, :, :3], vals[a], origins[a], vs)
        want[a, :, :3] = pts
        if stop[a] <= N:   # stopped because the reference runs out of the local grid (not into an obstacle inside it)?
            c = ((full[a, stop[a], :3] - origins[a]) / vs).astype(int)
            ctx.count["ref_past_grid"] += int(not all(0 <= c[k] < dim[k] for k in range(3)))
        want[a, :, 3:] = refmath.reference_velocities(pts, float(pv[a]))
    return want, pv, stop, caps, segs


def check_reference(ctx, pre, post, pre_plans, pre_has, tag=""):
    N = ctx.prm.n_hor
    want, pv, stop, caps, segs = expected_reference(ctx, pre, pre_plans, pre_has)
    for a in range(len(pre)):
        got = arr(post[a].traj_ref, co.MAXH + 1, 6)[:N + 1]
        assert post[a].n_ref == N + 1, (tag, a, post[a].n_ref)
        assert abs(post[a].path_vel - pv[a]) <= 1e-10 * max(1.0, abs(pv[a])), (tag, a, post[a].path_vel, pv[a])
        err = np.abs(got - want[a]) / np.maximum(1.0, np.abs(want[a]))
        assert err.max() <= 1e-10, (tag, a, int(stop[a]), float(err.max()), np.argwhere(err > 1e-10)[:4].tolist())
        s = int(stop[a])
        if s <= N:   # the stopping index exactly: from it on the point before it, bit for bit
            assert all(np.array_equal(got[i, :3], got[s - 1, :3]) for i in range(s, N + 1)), (tag, a, s)
            ctx.count["kept_free_stops"] += 1
        ctx.count["cap_lowered"] += int(caps[a] < ctx.cfg.path_vel_max - 1e-6)
        # the classes of polylines the segment masking of k_vel_cap has to get right
        lim = [v for v, _ in segs[a]]
        hit = [i for i, (_, c) in enumerate(segs[a]) if c]
        if hit and hit[0] >= 2:   # a collision on the third segment or later ...
            ctx.count["seg_collision_late"] += 1
            # ... behind a segment that crossed a weaker halo (its limit is lowered, but less than the collision's)
            ctx.count["seg_weak_before"] += int(any(ctx.cfg.path_vel_max - 1e-6 > v > lim[hit[0]] for v in lim[:hit[0]]))
        if hit and min(lim[hit[0] + 1:], default=np.inf) < caps[a] - 1e-6:   # a segment BEHIND the collision would lower the cap
            ctx.count["seg_masked_stronger"] += 1
    return segs


def check_commit(ctx, pre, post, plans, has, status, solver_out=None, tol=0.0, tag=""):
    """k_commit / commit_one from the state before the round and the round's own status. plans / has: the records the round
    published, indexed by agent id. solver_out: traj / ctrl / used of a solve of the same inputs (compared within tol; used exactly)."""
    N, P, step = ctx.prm.n_hor, ctx.prm.poly_hor, ctx.cfg.step_plan
    for a in range(len(pre)):
        p, q, rec = pre[a], post[a], plans[ctx.first_id + a]
        t_pre, c_pre = arr(p.traj_curr, co.MAXH + 1, 9), arr(p.ctrl_curr, co.MAXH, 3)
        t_post, c_post = arr(q.traj_curr, co.MAXH + 1, 9), arr(q.ctrl_curr, co.MAXH, 3)
        used_pre, used_post = np.array(p.poly_used[:], np.uint8), np.array(q.poly_used[:], np.uint8)
        ctx.count["agent_rounds"] += 1
        # what no phase of a round may touch
        assert (q.id, q.n_path) == (p.id, p.n_path) and bytes(q.path) == bytes(p.path) and bytes(q.goal) == bytes(p.goal), (tag, a)
        assert np.array_equal(t_post[N + 1:], t_pre[N + 1:]) and np.array_equal(c_post[N:], c_pre[N:]), (tag, a, "rows past the horizon")
        assert np.array_equal(used_post[P:], used_pre[P:]), (tag, a)
        if status[a] != NO_SOLUTION:
            ctx.count["solved"] += 1
            assert q.has_traj == 1 and has[ctx.first_id + a] == 1 and q.n_fail == p.n_fail, (tag, a)
            assert np.array_equal(t_post[:N + 1], rec), (tag, a, "traj_curr is the published record")
            if solver_out is not None:
                assert np.abs(t_post[:N + 1] - solver_out["traj"][a]).max() <= tol, (tag, a)
                assert np.abs(c_post[:N] - solver_out["ctrl"][a]).max() <= tol, (tag, a)
                assert np.array_equal(used_post[:P], solver_out["used"][a]), (tag, a)
        else:
            want_t, want_c, want_u = refmath.read_back(t_pre[:N + 1] if p.has_traj else None, c_pre[:N] if p.has_traj else None,
                                                       used_pre, None, None, None, failed=True)
            assert q.n_fail == p.n_fail + 1 and q.has_traj == p.has_traj, (tag, a)
            assert np.array_equal(used_post, want_u), (tag, a, "poly_used is kept")
            if p.has_traj:
                ctx.count["failed_with_plan"] += 1
                assert np.array_equal(t_post[:N + 1], want_t), (tag, a, "shift of traj_curr", np.argwhere(t_post[:N + 1] != want_t)[:4].tolist())
                assert np.array_equal(c_post[:N], want_c), (tag, a, "shift of ctrl_curr", np.argwhere(c_post[:N] != want_c)[:4].tolist())
                assert has[ctx.first_id + a] == 1 and np.array_equal(rec, want_t), (tag, a)
            else:
                # (on the wire the record carries a NaN in element 0 in place of the flag; a download hands it out as 0)
                ctx.count["failed_without_plan"] += 1
                assert has[ctx.first_id + a] == 0 and not rec.any(), (tag, a)
                assert np.array_equal(t_post, t_pre) and np.array_equal(c_post, c_pre), (tag, a)
                assert bytes(q.state_curr) == bytes(p.state_curr) and q.increment == p.increment, (tag, a)
                continue
        assert np.array_equal(arr(q.state_curr, 9), t_post[step]), (tag, a, "state_curr = traj_curr[step_plan]")
        ref = arr(q.traj_ref, co.MAXH + 1, 6)[:N + 1, :3]
        inc, _, d0 = refmath.reference_increment(t_post[1, :3], ref, ctx.cfg.thresh_dist)
        best = refmath.walk_minimum(t_post[1, :3], ref)
        guard = increment_guard(t_post[1, :3])
        if abs(best - d0) <= guard or abs(best - ctx.cfg.thresh_dist) <= guard:
            ctx.count["inc_left_out"] += 1
            continue
        assert q.increment == inc, (tag, a, q.increment, inc, best, d0)
        ctx.count["inc1" if inc else "inc0"] += 1


def check_round(ctx, pre, post, pre_plans, pre_has, plans, has, status, solver_out=None, tol=0.0, tag=""):
    """Every phase of one round (the packing is compared by the caller: with shard.inp on the host, through a second solver
    on the device). pre / post: AgentS arrays before and after; pre_plans / pre_has and plans / has: the records before and after."""
    check_corridor(ctx, pre, post, tag)
    check_reference(ctx, pre, post, pre_plans, pre_has, tag)
    check_commit(ctx, pre, post, plans, has, status, solver_out, tol, tag)


# ---- flights: a host-mirror loop driven by the oracle (the CPU test flies it, the device test takes its shard over) ----
def make_flight(oracle, shape, shift=(0.0, 0.0, 0.0), seed=0, starts=None, goals=None, route=True, rank=0, world=1, allgather=None):
    """(ctx, loop): SwarmLoop of the 16 agents in the world of make_world, the oracle as solver and as reference; rank / world /
    allgather: the loop of one block of the ceil split (starts / goals are the whole swarm's)."""
    prm, cfg = shape_params(shape)
    grid, worigin = make_world(shift)
    if starts is None:
        starts, goals = make_scene(seed, shift)
    ctx = Round(oracle, prm, cfg, grid, worigin, len(starts), first_id=swarm.shard_range(len(starts), rank, world)[0])

    def solve(inp, plans, has):
        return oracle.replan(prm, inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has,
                             n_threads=8)

    def ref_fn(ids, path, n_path, plans, has, vel_cap=None):
        full, _, pv = oracle.reference(prm, ctx.rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    loop = swarm.SwarmLoop(prm, cfg, len(starts), rank=rank, world=world, solve=solve, allgather=allgather, reference=ref_fn,
                           starts=starts, goals=goals)
    assert loop.set_world(grid, worigin, route=route) == 0
    loop.pmax = 32
    return ctx, loop


def host_rounds(ctx, loop, rounds, tag):
    """`rounds` rounds of the host mirror, every phase of each checked; the packing (fill_inputs) against the numpy rebuild bit for bit."""
    for r in range(rounds):
        pre = co.export_agents(loop.shard)[0]
        pre_plans, pre_has = loop.plans_all.copy(), loop.has_plan.copy()
        out = loop.step()
        post = co.export_agents(loop.shard)[0]
        check_round(ctx, pre, post, pre_plans, pre_has, loop.plans_all, loop.has_plan, out["status"], solver_out=out, tol=0.0, tag=(tag, r))
        want = rebuild_inputs(ctx.prm, pre, post)
        for key, v in want.items():
            assert np.array_equal(loop.shard.inp[key], v), (tag, r, key)
    return ctx.count


# ---- crafted states: a flight whose states were edited field by field before the round that is checked ----
SHIFT_FAR = (9999.9, 0.0, 0.0)   # +1e4 m in x, rounded to a whole number of voxels (hdsm_swarm_set_world wants the origin on the voxel lattice)


def crafted_startup_failure(oracle):
    """A first round — nobody has a plan of its own yet (has_traj = 0) — in which the solve of some agents fails: a block of 8 agents
    1.0 m apart and a block 3.0 m apart, each block swapping places; the plans that two rounds flown before have published stay
    in plans_all and cross the agents' ways, the agents themselves start again (no plan, no corridor)."""
    starts = np.array([[12.0 + 1.0 * (k % 4), 2.0 + 1.0 * (k // 4), 1.5] for k in range(8)] +
                      [[6.0 + 3.0 * (k % 4), 12.0 + 3.0 * (k // 4), 1.5] for k in range(8)])
    goals = np.concatenate([starts[:8][::-1], starts[8:][::-1]]) + [0.3, 0.2, 0.0]
    ctx, loop = make_flight(oracle, SHAPES[0], starts=starts, goals=goals, route=False)
    for _ in range(2):
        loop.step()
    buf = co.export_agents(loop.shard)[0]
    for a in range(N_AGENTS):
        buf[a].has_traj, buf[a].n_poly = 0, 0
    import_agents(loop.shard, buf)
    return ctx, loop


def crafted_shift_edge(oracle, shape):
    """A failure with a previous plan whose every element is distinct: every agent of a fresh flight is given a plan (has_traj = 1)
    whose traj_curr / ctrl_curr (all MAXH + 1 / MAXH rows, the ones past the horizon too) are an arange, and half of the agents a
    speed no input can bring back into the velocity box at x_1 (100 m/s against 20): their solve has no solution and the plan is
    shifted."""
    starts, goals = open_scene()
    ctx, loop = make_flight(oracle, shape, starts=starts, goals=goals, route=False)
    buf = co.export_agents(loop.shard)[0]
    for a in range(N_AGENTS):
        buf[a].has_traj = 1
        t = np.arange((co.MAXH + 1) * 9, dtype=np.float64) + 1000.0 * a + 0.5
        c = -(np.arange(co.MAXH * 3, dtype=np.float64) + 1000.0 * a + 0.25)
        C.memmove(buf[a].traj_curr, t.ctypes.data, t.nbytes)
        C.memmove(buf[a].ctrl_curr, c.ctypes.data, c.nbytes)
        if a % 2 == 0:
            buf[a].state_curr[5] = 100.0
    import_agents(loop.shard, buf)
    return ctx, loop


def crafted_paths(oracle):
    """Global paths of 1, 2, 5 and PATH_PTS points (set_paths; the single point through the state, which set_paths refuses), among
    them polylines that meet a pillar on their third segment or later after crossing a halo, and polylines that go on through a
    stronger halo or another pillar BEHIND the collision (k_vel_cap masks the lanes behind the first collision)."""
    rng = np.random.default_rng(5)
    ctx, loop = make_flight(oracle, SHAPES[0], route=False)
    starts = make_scene(0)[0]
    centres = np.array([[WORLD_ORIGIN[0] + (i + 0.5) * 0.3, WORLD_ORIGIN[1] + (j + 0.5) * 0.3] for i, j in PILLARS])
    paths, n_path = np.zeros((N_AGENTS, co.PATH_PTS, 3)), np.zeros(N_AGENTS, np.int32)
    for a in range(N_AGENTS):
        s = starts[a]
        if a % 4 == 1:       # two points: straight at the nearest pillar
            pts = [s, np.append(centres[np.argmin(np.linalg.norm(centres - s[:2], axis=1))], s[2])]
        elif a % 4 == 2:     # PATH_PTS points: a zig-zag through the pillars
            x = np.linspace(s[0], s[0] + (16.0 if s[0] < 14 else -16.0), co.PATH_PTS)
            pts = [np.array([x[i], s[1] + (0.8 if i % 2 else -0.8) * min(i, 3), s[2]]) for i in range(co.PATH_PTS)]
            pts[0] = s
        else:                # five points: past a pillar at halo distance twice, then into one, then on through the next ones
            near = centres[np.argsort(np.linalg.norm(centres - s[:2], axis=1))[:3]]
            off = rng.uniform(0.75, 1.3, 2)
            pts = [s, np.append(near[0] + [0.0, off[0]], s[2]), np.append(near[1] + [0.0, -off[1]], s[2]), np.append(near[2], s[2]),
                   np.append(near[0] + [0.3, 0.6], s[2])]
        n_path[a] = len(pts)
        paths[a, :len(pts)] = pts
    loop.shard.set_paths(paths, n_path)
    buf = co.export_agents(loop.shard)[0]
    for a in (0, 8):         # one point: the path is the start alone
        buf[a].n_path = 1
    import_agents(loop.shard, buf)
    return ctx, loop


def crafted_grid_edges(oracle):
    """Agents at the edges of what a local grid covers, at the H = 15 shape: one flying out of the world at path_vel_max (13.5 m of
    reference against the 10 m half-range of its grid: the reference is cut where the grid ends), two within two voxels of the
    world's border, two low enough that most of their grid lies below grid_z_min."""
    starts, goals = open_scene()
    starts[0], goals[0] = [31.0, 27.0, 1.5], [70.0, 27.0, 1.5]          # out of the world (free there), nothing near: no cap
    starts[1], goals[1] = [-2.6, 4.0, 1.5], [-2.6, 26.0, 1.5]            # along the world's x border, 0.4 m inside
    starts[2], goals[2] = [10.0, 29.6, 1.5], [28.0, 29.5, 1.5]           # ... the y border
    starts[3], goals[3] = [6.0, 1.0, 0.35], [25.0, 1.0, 0.35]            # just above the ground
    starts[4], goals[4] = [30.0, 1.0, 0.1], [8.0, 2.0, 0.4]
    return make_flight(oracle, H15_PLAIN, starts=starts, goals=goals, route=False)
