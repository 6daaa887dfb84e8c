"""Inputs for row f1 (k_ref_pack + k_reference<64|256>, hdsm_reference / hdsm_reference_device) at the shapes where the kernel
takes another path: the survivor list drained in mid-scan, instances that are a shuffled subset of the swarm, neighbour groups
whose range starts above 0, polylines beyond the 64 points kept in LDS, path counts that only the device entry clamps, non-finite
published plans, configurations that take the pairwise branch, and the edges of SamplePath and of the velocity row.

Shared by tests/test_reference_row.py (the oracle's orc_reference against refmath.reference_row, and the conditions on these
inputs) and tests/test_gpu_reference_row.py (the kernel against orc_reference). One generator of plans serves all cases: positions
plus a constant velocity over steps 0..N, no polyhedra. Every coordinate stays within 100 m of the origin, so the row's relative
tolerance 1e-10 * max(1, |y|.max()) is at most 1e-8 m in absolute terms.

Every case is built once per process (case(name)), its rendering by refmath.reference_row once (Case.render()); nobody writes to
either. An instance whose rendering takes a decision closer than the margins below is given a new path from the next seed — it is
redrawn, never dropped."""
import numpy as np

import refmath
from multi_agent_pkgs_amd.params import agile_ref_config, make_params

WALK_MARGIN = 1e-7   # |dist_next - limit| of every comparison of SamplePath's walk, outside the exact-landing case
VEL_MARGIN = 1e-6    # |dist - 1e-2| of every velocity row
SURV_CAP = 2048      # capacity of the kernel's survivor list (reference_kernels.hip)
GROUPS = (0, 70, 2131)  # + n_rob: [0, 70), [70, 2131) (2061 ids: one drain inside a range that starts above 0), [2131, n_rob)


class Case:
    """One call of the row. caps: the vel_cap of the call under comparison (None or [n_inst]); groups: hdsm_set_groups argument
    or None; n_path_device: what a device caller passes where it differs from n_path (the entry clamps it to n_path);
    special: {instance index: neighbour id} pairs the conditions speak about; exact: the exact-landing case."""

    def __init__(self, name, n_hor, cfg_kw, agent_id, path, n_path, plans, has_plan, caps=None, groups=None, dt=0.1,
                 n_path_device=None, special=None, exact=False, tight=False):
        self.name, self.n_hor, self.dt, self.cfg_kw = name, n_hor, dt, dict(cfg_kw)
        self.agent_id, self.n_path = np.asarray(agent_id, np.int32), np.asarray(n_path, np.int32)
        self.path, self.plans, self.has_plan = np.asarray(path, float), plans, np.asarray(has_plan, np.uint8)
        self.caps, self.groups, self.n_path_device = caps, groups, n_path_device
        self.special, self.exact, self.tight = dict(special or {}), exact, tight
        self._render = {}

    n_inst = property(lambda s: len(s.agent_id))
    n_rob = property(lambda s: len(s.has_plan))
    nt = property(lambda s: 64 if s.n_inst >= 256 else 256)   # the launch form hdsm_reference_device picks

    def prm(self):
        return make_params(n_hor=self.n_hor, dt=self.dt, max_rows_static=18)

    def cfg(self):
        return agile_ref_config(**self.cfg_kw)

    def ranges(self):
        """[n_inst][2]: the id range of every instance's group ((0, 0) behind the partition), None without groups"""
        if self.groups is None:
            return None
        table = np.zeros((self.n_rob, 2), np.int64)
        for lo, hi in zip(self.groups[:-1], self.groups[1:]):
            table[lo:hi] = (lo, hi)
        return table[self.agent_id]

    def other_caps(self):
        """the vel_cap of the second call a handle gets: a drawn one where the case has none, none where it has one"""
        return np.random.default_rng(9).uniform(3.0, 12.0, self.n_inst) if self.caps is None else None

    def render(self, only=None, has_plan=None, other=False):
        """refmath.reference_row on the case under caps (other: under other_caps()), cached; or on the instances `only` / with other
        has_plan flags (not cached)"""
        if only is None and has_plan is None and other in self._render:
            return self._render[other]
        sel = slice(None) if only is None else np.asarray(only)
        rg, caps = self.ranges(), self.other_caps() if other else self.caps
        out = refmath.reference_row(self.n_hor, self.dt, self.cfg(), self.agent_id[sel], self.path[sel], self.n_path[sel], self.plans,
                                    self.has_plan if has_plan is None else has_plan, None if caps is None else caps[sel],
                                    None if rg is None else rg[sel])
        if only is None and has_plan is None:
            self._render[other] = out
        return out

    def masked_calls(self):
        """The case as calls that know no groups: [(instance indices, has_plan masked to their range)]"""
        if self.groups is None:
            return [(np.arange(self.n_inst), self.has_plan)]
        calls, rg = [], self.ranges()
        for lo, hi in sorted({(int(a), int(b)) for a, b in rg}):
            m = np.zeros_like(self.has_plan)
            m[lo:hi] = self.has_plan[lo:hi]
            calls.append((np.nonzero((rg[:, 0] == lo) & (rg[:, 1] == hi))[0], m))
        return calls


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def linear_plans(rng, n_rob, n_hor, dt, half, speed=3.0):
    """[n_rob][N + 1][9]: positions uniform in the cube of half-width `half`, a constant velocity of about `speed` m/s"""
    plans = np.zeros((n_rob, n_hor + 1, 9))
    vel = rng.normal(size=(n_rob, 3)) * speed / np.sqrt(3.0)
    place(plans, np.arange(n_rob), rng.uniform(-half, half, (n_rob, 3)), vel, dt)
    return plans


def place(plans, k, p0, vel, dt):
    steps = np.arange(plans.shape[1]) * dt
    plans[k, :, :3] = np.asarray(p0, float)[..., None, :] + np.asarray(vel, float)[..., None, :] * steps[:, None]
    plans[k, :, 3:6] = np.asarray(vel, float)[..., None, :]


def random_path(rng, start, pmax):
    """a polyline from `start`: legs of a metre or two, mostly level"""
    pts = np.zeros((pmax, 3))
    pts[0] = start
    pts[1:] = start + np.cumsum(rng.normal(size=(pmax - 1, 3)) * [1.2, 1.2, 0.15], axis=0)
    return pts


def dense_path(rng, start, pmax, spacing=0.1, duplicates=False):
    """points about `spacing` apart (within a fifth of it: at exactly 0.1 m a cap of 5.0 m/s would land on every fifth point) along
    a gently turning line; duplicates: every fifth point repeats the one before it"""
    d = rng.normal(size=3)
    pts = np.zeros((pmax, 3))
    pts[0] = start
    for i in range(1, pmax):
        d = d + 0.15 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        pts[i] = pts[i - 1] if duplicates and i % 5 == 0 else pts[i - 1] + spacing * rng.uniform(0.8, 1.2) * d
    return pts


def settle(c, draw, seed):
    """Redraw (draw(k, seed) -> path) every instance whose rendering decides closer than the margins, with the next seed, until
    none is left — under the case's vel_cap and under the other choice, the two calls every handle of the GPU test gets. The
    renderings of the settled case are cached on it."""
    outs = {other: c.render(other=other) for other in (False, True)}
    for attempt in range(1, 50):
        bad = sorted({k for out in outs.values() for k, f in enumerate(out[3])
                      if min(f["walk"], default=1.0) <= WALK_MARGIN or min(f["vel"], default=1.0) <= VEL_MARGIN})
        if not bad:
            return c
        for k in bad:
            c.path[k] = draw(k, seed + attempt)
        for other, out in outs.items():
            new = c.render(only=bad, other=other)
            for n, k in enumerate(bad):
                out[0][k], out[1][k], out[2][k], out[3][k] = new[0][n], new[1][n], new[2][n], new[3][n]
    raise AssertionError(f"{c.name}: instances {bad} still decide inside the margins after 49 redraws")


def subset_ids(rng, n_inst, n_rob, must):
    must = sorted({m for m in must if 0 <= m < n_rob})
    rest = rng.choice(np.setdiff1d(np.arange(n_rob), must), n_inst - len(must), replace=False)
    ids = np.concatenate([must, rest]).astype(np.int32)
    rng.shuffle(ids)
    return ids


# ---- capacity ---------------------------------------------------------------------------------------------------------------------
CAPACITY_SHAPES = [(256, 2048), (256, 2049), (256, 2561), (8, 2049), (8, 4097)]


def _capacity(n_inst, n_rob, n_hor, form, seed):
    """form: 'tight' (cube of half-width 3 m: every sphere overlaps every other), 'sparse' (60 m, with the crafted instances),
    'grouped' (the tight ball under GROUPS)."""
    rng = np.random.default_rng(seed)
    dt, tight = 0.1, form != "sparse"
    plans = linear_plans(rng, n_rob, n_hor, dt, 3.0 if tight else 60.0)
    last = n_rob - 1
    # (instance agent, neighbour, offset) triples: the agent flies `offset` beside the neighbour, so that ids at, behind and far
    # behind the list's capacity set a path_vel whatever the draw. Under GROUPS the capacity counts from the range's first id, 70:
    # thirteen ids lie behind it, and with 256 instances two instances fly either side of each of them (a tenth of the instances).
    side = np.array([0.0, 0.01, 0.0])
    cluster = form == "tight" and (n_inst, n_rob) == (256, 2049)
    if form == "grouped":
        lo = GROUPS[1]
        partners = [(100, lo + SURV_CAP - 1, side), (101, lo + SURV_CAP, side), (102, GROUPS[2] - 1, side)]
        if n_inst >= 64:
            partners = [partners[0]] + [(110 + 2 * n + e, nb, side * (1 - 2 * e)) for n, nb in enumerate(range(lo + SURV_CAP, GROUPS[2])) for e in (0, 1)]
    else:
        partners = [(a, nb, side) for a, nb in ((1, 2047), (2, 2048)) if nb < n_rob and not (cluster and nb == 2048)]
        partners += [(3, last, side)] if last > 2048 else []
    members = list(range(10, 46)) if cluster else []
    ids = subset_ids(rng, n_inst, n_rob, [0, 2047, 2048, last] + [a for a, _, _ in partners] + members)
    where = {int(a): k for k, a in enumerate(ids)}
    special = {}
    if tight:
        for a, nb, off in partners:
            place(plans, a, plans[nb, 0, :3] + off, plans[nb, 0, 3:6], dt)
            special[where[a]] = nb
        # agent 0 crosses the ball through its centre at 10 m/s: its sphere holds the whole ball, nearly every neighbour survives
        place(plans, 0, [-5.0 * n_hor * dt, 0.0, 0.0], [10.0, 0.0, 0.0], dt)
    if cluster:
        # 2049 agents: ONE id lies behind the capacity, and a tenth of 256 instances must hang on it. At most twelve points can sit
        # on a sphere around it and be further from each other than from its centre (the corners of an icosahedron: edge 1.05 r).
        # So agent 2048 stands at three places in turn, a third of the steps each, and twelve instances stand still 0.02 m around
        # each place: for each of the 36 the closest (neighbour, step) pair is agent 2048 while it is there.
        phi = 0.5 * (1.0 + np.sqrt(5.0))
        corners = np.array([np.roll([0.0, sy, sz * phi], ax) for ax in range(3) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]) / np.sqrt(1.0 + phi * phi)
        spots = np.array([[-1.0, 0.7, 0.3], [1.0, 0.5, -0.4], [0.2, -1.0, 1.0]])
        third = np.minimum(np.arange(n_hor + 1) * 3 // (n_hor + 1), 2)
        plans[2048, :, :3], plans[2048, :, 3:6] = spots[third], 0.0
        for n, a in enumerate(members):
            place(plans, a, spots[n // 12] + 0.02 * corners[n % 12], np.zeros(3), dt)
            special[where[a]] = 2048
    if not tight:
        # crafted instances of the sparse swarm: agent a far from everybody (a corner region of its own), its partner 0.5 m away
        for n, (a, nb, _) in enumerate(partners):
            spot, vel = np.array([75.0, -75.0 + 20.0 * n, 70.0]), np.array([1.0, 2.0, 0.5])
            place(plans, a, spot, vel, dt)
            place(plans, nb, spot + [0.0, 0.5, 0.0], vel, dt)
            special[where[a]] = nb
        # agent 0 stands still; agent 4 (jstar: its sphere holds agent 0, its steps stay 2 m away) and agent 5 (the setter: a long
        # plan that comes within 0.3 m at the last step but one)
        spot, T = np.array([-75.0, 75.0, 70.0]), n_hor * dt
        place(plans, 0, spot, [0.0, 0.0, 0.0], dt)
        place(plans, 4, spot + [-10.0 * T, 2.0, 0.0], [20.0, 0.0, 0.0], dt)
        place(plans, 5, spot + [0.0, -18.0 * (n_hor - 1) * dt, 0.3], [0.0, 18.0, 0.0], dt)
        special[where[0]] = 5
    has = np.ones(n_rob, np.uint8)
    pmax = 12

    def draw(k, s):
        return random_path(np.random.default_rng([seed, int(ids[k]), s]), plans[ids[k], 0, :3], pmax)

    path = np.array([draw(k, 0) for k in range(n_inst)])
    n_path = np.full(n_inst, pmax, np.int32)
    n_path[::9] = 2
    groups = list(GROUPS) + [n_rob] if form == "grouped" else None
    c = Case(f"{form}-i{n_inst}-r{n_rob}-h{n_hor}", n_hor, {}, ids, path, n_path, plans, has, groups=groups, special=special,
             tight=tight)
    return settle(c, draw, 0)


def sphere_stats(c):
    """Host-side restatement of the kernel's cull for the statistics and the conditions (never for an expected value): per
    instance the closest sphere jstar, the survivors of the sphere test, and how many of them lie among the first SURV_CAP ids of
    the instance's range (what one filling of the list holds)."""
    pos = c.plans[:, :, :3]
    with np.errstate(all="ignore"):
        ctr = 0.5 * (np.fmin.reduce(pos, axis=1) + np.fmax.reduce(pos, axis=1))
        rad = np.sqrt(((pos - ctr[:, None]) ** 2).sum(2).max(1)) * (1 + 1e-9)
    rad[~np.isfinite(rad) | ~(rad < 1e299)] = 1e300
    rad[c.has_plan == 0] = -1.0
    rg = c.ranges()
    jstar, surv, first = np.full(c.n_inst, -1), np.zeros(c.n_inst, int), np.zeros(c.n_inst, int)
    for k, me in enumerate(c.agent_id):
        lo, hi = (0, c.n_rob) if rg is None else rg[k]
        if not (0 <= me < c.n_rob) or not c.has_plan[me] or hi <= lo:
            continue
        js = np.array([j for j in range(lo, hi) if j != me and rad[j] >= 0])
        if js.size == 0:
            continue
        with np.errstate(all="ignore"):
            gap = np.sqrt(((ctr[js] - ctr[me]) ** 2).sum(1)) - rad[js] - rad[me]
            jstar[k] = js[np.nanargmin(gap)] if np.isfinite(gap).any() or (gap == gap).any() else -1
            u = ((pos[me] - pos[jstar[k]]) ** 2).sum(1) if jstar[k] >= 0 else np.zeros(1)
            umax = np.where(u == u, u, np.finfo(float).max).max()
            reach = rad[js] + rad[me] + np.sqrt(umax) * (1 + 1e-9)
            keep = ~(((ctr[js] - ctr[me]) ** 2).sum(1) > reach * reach * (1 + 1e-9))
        surv[k], first[k] = keep.sum(), keep[js < lo + SURV_CAP].sum()
    return dict(jstar=jstar, survivors=surv, first_filling=first)


# ---- polylines --------------------------------------------------------------------------------------------------------------------
PMAX = 80
N_PATHS = (1, 2, 63, 64, 65, 80)
CAPS = (0.0, 0.05, 0.11, 5.0, 50.0)   # 0.05 and 0.11: sample points 0.005 m and 0.011 m apart, either side of the row's 1e-2


def _polyline(n_inst, n_hor, dec, seed):
    """Every n_path of N_PATHS, a path that ends after three steps' worth (21 points: 2 m) and one with duplicate points, each under
    every cap of CAPS (and, in the second call of the GPU test, under none); points 0.1 m apart. A few neighbours 1.5-4 m away."""
    rng = np.random.default_rng(seed)
    n_rob = n_inst + 8
    plans = linear_plans(rng, n_rob, n_hor, 0.1, 20.0, speed=1.0)
    ids = subset_ids(rng, n_inst, n_rob, [0, n_rob - 1])
    kinds = [(n, False) for n in N_PATHS] + [(21, False), (PMAX, True)]
    n_path, dup, caps = np.zeros(n_inst, np.int32), np.zeros(n_inst, bool), np.zeros(n_inst)
    for k in range(n_inst):
        (n_path[k], dup[k]), caps[k] = kinds[k % len(kinds)], CAPS[(k // len(kinds)) % len(CAPS)]

    def draw(k, s):
        return dense_path(np.random.default_rng([seed, k, s]), plans[ids[k], 0, :3], PMAX, duplicates=bool(dup[k]))

    path = np.array([draw(k, 0) for k in range(n_inst)])
    c = Case(f"polyline-i{n_inst}-h{n_hor}-dec{dec:g}", n_hor, dict(path_vel_dec=dec), ids, path, n_path, plans,
             np.ones(n_rob, np.uint8), caps=caps)
    return settle(c, draw, 0)


def _exact_landing():
    """dt = 0.125 and path points at multiples of 0.5 m along an axis: every quantity of the walk is a dyadic number, so the walk is
    exact in double and in long double alike. No instance has a neighbour with a plan: path_vel is the cap alone (5.0: the walk
    lands on a path point with nothing left at every fourth sample; 4.0: at every sample; 2.0: at every second)."""
    n_hor, dt, n_rob = 10, 0.125, 4
    plans = np.zeros((n_rob, n_hor + 1, 9))
    place(plans, np.arange(n_rob), [[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 8.0]], np.zeros((n_rob, 3)), dt)
    has = np.array([1, 0, 0, 0], np.uint8)           # instance 0: a plan of its own and nobody else's; the others: no plan of their own
    path = np.zeros((4, PMAX, 3))
    for k, ax in enumerate((0, 1, 2, 0)):
        path[k] = plans[k, 0, :3]
        path[k, :, ax] += 0.5 * np.arange(PMAX) * (-1.0 if k == 3 else 1.0)
    return Case("exact-landing", n_hor, {}, np.arange(4), path, [80, 64, 65, 12], plans, has, caps=np.array([5.0, 5.0, 4.0, 2.0]),
                dt=dt, exact=True)


def _clamp(seed=77):
    """n_path of 0, -3 and pmax + 5, which only hdsm_reference_device accepts: it clamps them to 1, 1 and pmax. The neighbours
    are 40 m away, so path_vel is about 8.4 m/s and the 8 m polyline runs out inside the 16-step horizon: a count above pmax would
    walk on into the next instance's polyline (the over-long count is never the last instance's)."""
    rng = np.random.default_rng(seed)
    n_hor, n_inst, n_rob = 16, 6, 6
    plans = np.zeros((n_rob, n_hor + 1, 9))
    place(plans, np.arange(n_rob), 40.0 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1.0]]), rng.normal(size=(n_rob, 3)), 0.1)

    def draw(k, s):
        return dense_path(np.random.default_rng([seed, k, s]), plans[k, 0, :3], PMAX)

    path = np.array([draw(k, 0) for k in range(n_inst)])
    device = np.array([0, -3, PMAX + 5, PMAX, PMAX + 5, 65], np.int32)
    c = Case("clamp", n_hor, {}, np.arange(n_inst), path, np.clip(device, 1, PMAX), plans, np.ones(n_rob, np.uint8), n_path_device=device)
    return settle(c, draw, 0)


# ---- configurations ---------------------------------------------------------------------------------------------------------------
CONFIGS = {"sens_dist_negative": dict(sens_dist=-0.2, sens_other_agents=0.8),          # not monotone in the distance: pairwise branch
           "vel_max_below_min": dict(path_vel_max=4.0, path_vel_min=6.0),               # pairwise branch too
           "fading": dict(sens_other_agents=0.8, path_vel_dec=0.5),                     # the list branch, weights that fall with the step
           "plain": dict(sens_other_agents=1.0)}


def _config(which, n_inst, seed=11, beyond=False):
    """300 agents in a cube of half-width 5 m under the configuration CONFIGS[which]; n_inst of them are instances. A tenth have no
    plan (instances among them), agents 5 and 6 are coincident, agents 8 and 9 stand at exactly equal distances either side of
    agent 7. beyond: a partition of 297 agents under n_rob = 300 — the instances with ids 298 and 299 lie behind it and meet nobody.
    (With path_vel_max < path_vel_min every limit lies between the two and the cap never exceeds the lower one: the neighbour
    term runs, pair by pair, and never bites.)"""
    rng = np.random.default_rng(seed)
    n_hor, n_rob, pmax = 10, 300, 5
    plans = linear_plans(rng, n_rob, n_hor, 0.1, 5.0)
    has = (rng.random(n_rob) >= 0.1).astype(np.uint8)
    has[[5, 6, 7, 8, 9]] = 1
    plans[6] = plans[5]
    place(plans, 7, [8.0, 8.0, 8.0], [0.0, 0.0, 0.0], 0.1)          # standing still, dyadic numbers: the two distances are equal to the bit
    place(plans, 8, [8.0, 8.5, 8.0], [0.0, 0.0, 0.0], 0.1)
    place(plans, 9, [8.0, 7.5, 8.0], [0.0, 0.0, 0.0], 0.1)
    has[[298, 299]] = 1
    absent = np.nonzero(has == 0)[0]
    must = [5, 6, 7, 8, int(absent[0]), int(absent[1]), 0, n_rob - 1] + ([298, 299] if beyond else [])
    ids = np.arange(n_rob, dtype=np.int32) if n_inst == n_rob else subset_ids(rng, n_inst, n_rob, must)
    if n_inst == n_rob:
        rng.shuffle(ids)

    def draw(k, s):
        return random_path(np.random.default_rng([seed, int(ids[k]), s]), plans[ids[k], 0, :3], pmax)

    path = np.array([draw(k, 0) for k in range(n_inst)])
    n_path = np.full(n_inst, pmax, np.int32)
    n_path[::7], n_path[3] = 2, 1
    c = Case(f"{which}-i{n_inst}" + ("-beyond" if beyond else ""), n_hor, CONFIGS[which], ids, path, n_path, plans, has,
             caps=np.random.default_rng(seed + 1).uniform(3.0, 12.0, n_inst), groups=[0, 150, 297] if beyond else None)
    return settle(c, draw, 0)


# ---- non-finite plans -------------------------------------------------------------------------------------------------------------
NONFINITE = ("a", "b", "c", "d", "e", "f")


def _nonfinite(letter, n_inst, n_rob, seed=23):
    """Agent T = 3 and a neighbour S = 10 that stays 0.4 m beside it over the whole horizon (everybody else is metres away),
    has_plan = 1 for both: (a) S has NaN at step 0 only; (b) one coordinate of S is +inf from step 2 on; (c) S has +inf at step 3
    and -inf at step 5: the centre of its sphere is NaN; (d) T's own plan has NaN at step 4, S is finite; (e) is (b) with S the only
    neighbour that has a plan. In each the finite steps of S set T's path_vel (special = {T's instance: S}).
    (f) is (c) with S 6 m away and a third plan, agent Q's, 3 m from T; nobody else has one, all three stand still (no two spheres
    overlap). The scans of T's workgroup meet Q in the same lane as S and after it (S = 10, Q = 266 = S + 4 * 64 = S + 256), and Q
    sets T's path_vel (special = {T's instance: Q})."""
    rng = np.random.default_rng(seed)
    n_hor, pmax, T, S, Q = 10, 4, 3, 10, 266
    plans = linear_plans(rng, n_rob, n_hor, 0.1, 12.0, speed=1.0)
    vel = np.array([0.5, -0.25, 0.125]) if letter != "f" else np.zeros(3)
    place(plans, T, [30.0, 30.0, 30.0], vel, 0.1)
    place(plans, S, [30.0, 30.4 if letter != "f" else 36.0, 30.0], vel, 0.1)
    has = np.ones(n_rob, np.uint8)
    if letter == "a":
        plans[S, 0, 0] = np.nan
    elif letter in ("b", "e"):
        plans[S, 2:, 1] = np.inf
    elif letter in ("c", "f"):
        plans[S, 3, 0], plans[S, 5, 0] = np.inf, -np.inf
    elif letter == "d":
        plans[T, 4, 2] = np.nan
    if letter in ("e", "f"):
        has[:] = 0
        has[[T, S]] = 1
    if letter == "f":
        place(plans, Q, [33.0, 30.0, 30.0], vel, 0.1)
        has[Q] = 1
    ids = np.arange(n_rob, dtype=np.int32) if n_inst == n_rob else subset_ids(rng, n_inst, n_rob, [T, S, 0, n_rob - 1])
    special = {int(np.nonzero(ids == T)[0][0]): Q if letter == "f" else S}

    def draw(k, s):
        start = plans[ids[k], 0, :3]
        return random_path(np.random.default_rng([seed, int(ids[k]), s]), start if np.isfinite(start).all() else np.zeros(3), pmax)

    path = np.array([draw(k, 0) for k in range(n_inst)])
    c = Case(f"nonfinite-{letter}-i{n_inst}-r{n_rob}", n_hor, {}, ids, path, np.full(n_inst, pmax, np.int32), plans, has, special=special)
    return settle(c, draw, 0)


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _builders():
    b = {}
    for n, (n_inst, n_rob) in enumerate(CAPACITY_SHAPES):
        for n_hor in (10, 16):
            b[f"tight-i{n_inst}-r{n_rob}-h{n_hor}"] = (_capacity, (n_inst, n_rob, n_hor, "tight", 100 + n))
        n_hor = (10, 16)[n % 2]
        b[f"sparse-i{n_inst}-r{n_rob}-h{n_hor}"] = (_capacity, (n_inst, n_rob, n_hor, "sparse", 200 + n))
        if n_rob > GROUPS[-1]:
            b[f"grouped-i{n_inst}-r{n_rob}-h{26 - n_hor}"] = (_capacity, (n_inst, n_rob, 26 - n_hor, "grouped", 300 + n))
    for n_inst, n_hor, dec in [(40, 16, 0.0), (40, 10, 0.5), (40, 16, 100.0), (280, 10, 0.5)]:
        b[f"polyline-i{n_inst}-h{n_hor}-dec{dec:g}"] = (_polyline, (n_inst, n_hor, dec, 400 + n_inst + n_hor))
    b["exact-landing"] = (_exact_landing, ())
    b["clamp"] = (_clamp, ())
    for which in CONFIGS:
        for n_inst in (300, 20):
            b[f"{which}-i{n_inst}"] = (_config, (which, n_inst))
    b["plain-i20-beyond"] = (_config, ("plain", 20, 11, True))
    for letter in NONFINITE:
        for n_inst, n_rob in ((17, 17), (300, 300), (20, 300)):
            if letter == "f" and n_rob < 267:
                continue
            b[f"nonfinite-{letter}-i{n_inst}-r{n_rob}"] = (_nonfinite, (letter, n_inst, n_rob))
    return b


BUILDERS = _builders()
NAMES = list(BUILDERS)
_built = {}


def case(name):
    if name not in _built:
        fn, args = BUILDERS[name]
        _built[name] = fn(*args)
        assert _built[name].name == name, (_built[name].name, name)
        assert np.nanmax(np.abs(np.where(np.isfinite(_built[name].plans[:, :, :3]), _built[name].plans[:, :, :3], 0.0))) <= 100.0
        assert np.abs(_built[name].path).max() <= 100.0
    return _built[name]


def names(family):
    return [n for n in NAMES if family_of(n) == family]


def family_of(name):
    head = name.split("-")[0]
    return {"tight": "capacity", "sparse": "capacity", "grouped": "capacity", "polyline": "polyline", "exact": "polyline", "clamp": "clamp",
            "nonfinite": "nonfinite"}.get(head, "config")
