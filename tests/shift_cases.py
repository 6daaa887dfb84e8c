"""Cases for the plan shifts of the solver handle (hdsm_set_plan_shift*, hdsm_set_own_plans_device; include/hdsm.h) and their
yardstick: the oracle called per instance on MATERIALISED records. With shift[k] = s every instance but k's own reads record k as
R'[i] = R[min(i + s, N)]; so the expected answer of agent a is what the oracle returns for a alone when every other record is
replaced by its R', a's own record is left as it is and — with the own-plan override — comes from the override's arrays.
tests/test_plan_shift.py asserts from the oracle alone that these cases can see a shift that is ignored; tests/test_gpu_plan_shift.py
runs them on the GPU.

16 agents in two rows of eight that fly at each other at 3 m/s (crossing_round): agent k of the first row passes agent k + 8 of the
second at 0.8 m, in the middle of the horizon, while both references lean into the other's lane — the plane against the partner is
active, and a partner advanced by a few steps puts it somewhere else. Shift values: 0, 1, N - 1, N, N + 3 (above N behaves as N)
and ages 1..4 times step_plan for step_plan 1 and 3 — what the device loop writes (age * step_plan). Agents 3 and 10 have no plan."""
import numpy as np

import problems
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

ARG_KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
N_ROB = 16
ABSENT = (3, 10)
CASES = [(n_hor, step_plan) for n_hor in (7, 10, 15) for step_plan in (1, 3)]
IDS = [f"h{h}-step{s}" for h, s in CASES]


def shifts(n_hor, step_plan):
    """the named values first, then ages times step_plan; one agent alone is unshifted"""
    named = [0, 1, n_hor - 1, n_hor, n_hor + 3]
    vals = named + [age * step_plan for age in (1, 2, 3, 4, 1)] + named[:0:-1] + [2 * step_plan, 3 * step_plan]
    assert len(vals) == N_ROB
    return np.asarray(vals, dtype=np.int32)


def crossing_round(prm, seed, pitch=2.4, lane=0.8, lean=1.2, v=3.0):
    """One replan round of the two rows: row one (agents 0..7, `pitch` apart in x) flies +y, row two (agents 8..15, `lane` to the side)
    flies -y from v dt N away; the records are straight lines at constant speed (jittered by the seed), the references lean by
    `lean` : 1 into the partner's lane, the corridor is one roomy box. Agents ABSENT have no plan."""
    N, P, RS, dt = prm.n_hor, prm.poly_hor, prm.max_rows_static, prm.dt
    rng = np.random.default_rng(seed)
    first = np.arange(N_ROB) < 8
    pos = np.stack([pitch * (np.arange(N_ROB) % 8) + np.where(first, 0.0, lane), np.where(first, 0.0, v * dt * N), np.full(N_ROB, 1.5)], axis=1)
    vel = np.stack([np.zeros(N_ROB), np.where(first, v, -v), np.zeros(N_ROB)], axis=1)
    lean_dir = np.stack([np.where(first, lean, -lean), np.where(first, 1.0, -1.0), np.zeros(N_ROB)], axis=1)
    pos += rng.uniform(-0.08, 0.08, (N_ROB, 3)) * [1, 1, 0.5]
    vel += rng.uniform(-0.2, 0.2, (N_ROB, 3)) * [1, 1, 0.2]
    plans = np.zeros((N_ROB, N + 1, 9))
    plans[:, :, :3] = pos[:, None, :] + vel[:, None, :] * dt * (np.arange(N + 1) - 1)[None, :, None]
    plans[:, :, 3:6] = vel[:, None, :]
    state = plans[:, 1].copy()
    ref = np.stack([problems.ref_from_path(state[k, :3], lean_dir[k], v, dt, N) for k in range(N_ROB)])
    n_poly, n_rows, A, b = problems.pack_static([[problems.box_rows(state[k, :3] - 6.0, state[k, :3] + 6.0)] for k in range(N_ROB)], P, RS)
    has = np.ones(N_ROB, np.uint8)
    has[list(ABSENT)] = 0
    return dict(agent_id=np.arange(N_ROB, dtype=np.int32), state=state, ref=ref, n_poly=n_poly, n_rows=n_rows, A=A, b=b, plans=plans, has_plan=has)


def materialise(plans, shift):
    """R'[k][i] = R[k][min(i + shift[k], N)]"""
    n, N = plans.shape[0], plans.shape[1] - 1
    s = np.minimum(np.maximum(np.asarray(shift, dtype=np.int64), 0), N)
    idx = np.minimum(np.arange(N + 1)[None, :] + s[:, None], N)
    return plans[np.arange(n)[:, None], idx]


def view_of(a, plans, has, shift, own_plans=None, own_has=None):
    """(plans_all, has_plan) as agent a's instance reads them"""
    m, h = materialise(plans, shift), np.array(has, dtype=np.uint8, copy=True)
    m[a] = (plans if own_plans is None else own_plans)[a]
    if own_has is not None:
        h[a] = own_has[a]
    return m, h


class Case:
    def __init__(self, n_hor, step_plan):
        self.n_hor, self.step_plan = n_hor, step_plan
        self.sn = crossing_round(self.prm(), seed=10 * n_hor + step_plan)
        self.shift = shifts(n_hor, step_plan)
        # the override batch: the own slots of plans_all hold a DECOY (every agent's record moved and bent), the true records are the
        # override; agent 5's flag is 0 in has_plan (the others do not see it) and 1 in the override (it flies its own plan)
        rng = np.random.default_rng(7 + n_hor)
        self.own_plans, self.own_has = self.sn["plans"], self.sn["has_plan"].copy()
        self.decoy = self.sn["plans"].copy()
        self.decoy[:, :, :3] += rng.uniform(0.4, 0.9, (N_ROB, 1, 3)) * rng.choice([-1.0, 1.0], (N_ROB, 1, 3)) * [1, 1, 0.3]
        self.decoy[:, :, :3] += np.linspace(0.0, 1.0, n_hor + 1)[None, :, None] * rng.uniform(-1.0, 1.0, (N_ROB, 1, 3))
        self.decoy_has = self.sn["has_plan"].copy()
        self.decoy_has[5] = 0
        # reference inputs (tests/test_gpu_groups.py): a three-point polyline from every agent's position
        self.path = np.zeros((N_ROB, 3, 3))
        self.path[:, 0] = self.sn["state"][:, :3]
        self.path[:, 1] = self.path[:, 0] + [6.0, 2.0, 0.0]
        self.path[:, 2] = self.path[:, 1] + [0.0, 30.0, 0.5]
        self.n_path = np.full(N_ROB, 3, np.int32)
        self._memo = {}

    def prm(self, **kw):
        return agile_params(self.n_hor, max_rows_static=18, **kw)

    def args(self, plans=None, has=None):
        return [self.sn[k] if k not in ("plans", "has_plan") else (plans if k == "plans" and plans is not None else has if k == "has_plan" and has is not None else self.sn[k])
                for k in ARG_KEYS]

    def _per_instance(self, oracle, views):
        outs = []
        for a in range(N_ROB):
            m, h = views(a)
            outs.append(oracle.replan(self.prm(), *[self.sn[k][a:a + 1] for k in ARG_KEYS[:7]], m, h))
        return {k: np.concatenate([o[k] for o in outs]) for k in ("traj", "ctrl", "status", "obj")}

    def want(self, oracle, which):
        """the oracle's answers: 'shifted' (the definition), 'unshifted' (the shift ignored), 'override' (shifted, decoy in plans_all,
        the true records through the override), 'decoy' (shifted, the decoy taken as the own record: the override ignored)"""
        if which not in self._memo:
            sn = self.sn
            views = {"shifted": lambda a: view_of(a, sn["plans"], sn["has_plan"], self.shift),
                     "unshifted": lambda a: (sn["plans"], sn["has_plan"]),
                     "override": lambda a: view_of(a, self.decoy, self.decoy_has, self.shift, self.own_plans, self.own_has),
                     "decoy": lambda a: view_of(a, self.decoy, self.decoy_has, self.shift)}[which]
            self._memo[which] = self._per_instance(oracle, views)
        return self._memo[which]

    def ref_cfg(self, monotone=True):
        # (not monotone in the distance — tests/reference_cases.py, "sens_dist_negative": k_reference reads the records directly)
        return agile_ref_config() if monotone else agile_ref_config(sens_dist=-0.2, sens_other_agents=0.8)

    def want_reference(self, oracle, monotone, override):
        key = ("ref", monotone, override)
        if key not in self._memo:
            sn, N = self.sn, self.n_hor
            full, ref, pv = np.zeros((N_ROB, N + 1, 6)), np.zeros((N_ROB, N, 6)), np.zeros(N_ROB)
            for a in range(N_ROB):
                m, h = (view_of(a, self.decoy, self.decoy_has, self.shift, self.own_plans, self.own_has) if override
                        else view_of(a, sn["plans"], sn["has_plan"], self.shift))
                full[a:a + 1], ref[a:a + 1], pv[a:a + 1] = oracle.reference(self.prm(), self.ref_cfg(monotone), sn["agent_id"][a:a + 1], self.path[a:a + 1],
                                                                            self.n_path[a:a + 1], m, h)
            self._memo[key] = (full, ref, pv)
        return self._memo[key]


_cases = {}


def case(idx):
    if idx not in _cases:
        _cases[idx] = Case(*CASES[idx])
    return _cases[idx]


def moved(a, b):
    """per instance: the largest distance between two answers' trajectories [m] (inf where exactly one has no solution)"""
    d = np.abs(a["traj"][:, :, :3] - b["traj"][:, :, :3]).reshape(len(a["status"]), -1).max(1)
    one = (a["status"] == 2) != (b["status"] == 2)
    both = (a["status"] == 2) & (b["status"] == 2)
    return np.where(one, np.inf, np.where(both, 0.0, d))


# ---- the sphere case: bounds must be those of the SHIFTED positions -------------------------------------------------------------
def sphere_case(n_hor=10):
    """Eight agents in a row 1.2 m apart that hover (every record a constant position) and a ninth, agent 8, whose record starts 40 m
    away and ends beside agent 0: steps 1..N run from far to near, so its UNSHIFTED sphere reaches from here to there and no
    instance can cull it, while shifted by N it is one point — beside agent 0 and provably slack for agents 4..7, whose prefilter
    then skips it without reading a position. Returns (prm kwargs, snapshot, shift)."""
    prm = agile_params(n_hor, max_rows_static=18)
    N, P, RS, dt = prm.n_hor, prm.poly_hor, prm.max_rows_static, prm.dt
    n = 9
    plans = np.zeros((n, N + 1, 9))
    for k in range(8):
        plans[k, :, :3] = [1.2 * k, 0.0, 1.5]
    far, near = np.array([40.0, 30.0, 1.5]), np.array([0.0, 1.1, 1.5])
    plans[8, :, :3] = far[None, :] + (near - far)[None, :] * (np.arange(N + 1) / N)[:, None] ** 3
    state = plans[:, 1].copy()
    # every reference hovers where its agent is, but agent 0's: it flies at 3 m/s towards the point where agent 8's record ends
    ref = np.stack([problems.ref_from_path(state[k, :3], np.array([0.0, 1.0, 0.0]), 3.0 if k == 0 else 0.0, dt, N) for k in range(n)])
    n_poly, n_rows, A, b = problems.pack_static([[problems.box_rows(state[k, :3] - 3.0, state[k, :3] + 3.0)] for k in range(n)], P, RS)
    sn = dict(agent_id=np.arange(n, dtype=np.int32), state=state, ref=ref, n_poly=n_poly, n_rows=n_rows, A=A, b=b, plans=plans,
              has_plan=np.ones(n, np.uint8))
    shift = np.zeros(n, np.int32)
    shift[8] = N
    return prm, sn, shift
