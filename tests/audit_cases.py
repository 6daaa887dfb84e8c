"""Cases and an independent numpy restatement of the flight audit (csrc/audit_core.h) for the flight-audit tests.

The restatement shares no code with the library. Separation: the ratio q = (dx^2 + dy^2) / (2 r)^2 + dz^2 / (2 z)^2 between two
agents that move linearly and synchronously through a sub-step, minimised over t in [0, 1] in closed form, vectorised over
(subject, sub-step, partner); numpy's argmin over the flattened (sub-step, partner) axis returns the first minimum, which is the
tie rule (smaller sub-step, then lower id). Own track: plain voxel look-ups and the statement-by-statement Python Raycast of
test_host.py. Accumulation: plain Python over the records of the rounds."""
import math

import numpy as np

from refmath import py_raycast as _py_raycast

N_HOR = 4          # horizon of the generated records (>= every step_plan used)
BIG = np.finfo(np.float64).max


def wdot(u, v, r, z):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) / (2 * r) ** 2 + u[..., 2] * v[..., 2] / (2 * z) ** 2


def pair_q(P, subj, S, r, z):
    """q [len(subj)][S][G]: the minimum over t of the ratio between subject and every agent in each sub-step; t* too."""
    a0, a1 = P[subj, :S, None, :], P[subj, 1:S + 1, None, :]               # [m][S][1][3]
    b0, b1 = P[None, :, :S, :].transpose(0, 2, 1, 3), P[None, :, 1:S + 1, :].transpose(0, 2, 1, 3)   # [1][S][G][3]
    d0, d1 = a0 - b0, a1 - b1
    e = d1 - d0
    ee, de = wdot(e, e, r, z), wdot(d0, e, r, z)
    t = np.where(ee > 0, np.clip(-de / np.where(ee > 0, ee, 1.0), 0.0, 1.0), 0.0)
    d = np.where((t >= 1.0)[..., None], d1, d0 + t[..., None] * e)            # (the end vector itself at t* = 1)
    return wdot(d, d, r, z), (d0, e, ee)


def np_separation(plans, has, S, first, n_local, r, z, block=128):
    """sep2, partner, substep for the subjects of the window, and two runners-up: the smallest q of any OTHER partner, and the
    smallest q of the same partner in another sub-step (inf where there is none)."""
    plans, has = np.asarray(plans, np.float64), np.asarray(has).astype(bool)
    G = plans.shape[0]
    P = plans[:, :S + 1, :3]
    sep2, partner, substep = np.full(n_local, BIG), np.full(n_local, -1, np.int32), np.zeros(n_local, np.int32)
    second, second_sub = np.full(n_local, np.inf), np.full(n_local, np.inf)
    for k0 in range(0, n_local, block):
        subj = np.arange(first + k0, first + min(n_local, k0 + block))
        q, _ = pair_q(P, subj, S, r, z)
        q = np.where(has[None, None, :], q, np.inf)
        q[np.arange(len(subj)), :, subj] = np.inf
        flat = q.reshape(len(subj), S * G)
        idx = np.argmin(flat, axis=1)
        best = flat[np.arange(len(subj)), idx]
        rows = np.arange(len(subj))
        same = q[rows, :, idx % G].copy()                                       # [m][S]: the winner's partner in every sub-step
        same[rows, idx // G] = np.inf
        others = q.copy()
        others[rows, :, idx % G] = np.inf
        for t, a in enumerate(subj):
            k = a - first
            if not has[a] or not np.isfinite(best[t]):
                continue
            sep2[k], partner[k], substep[k] = best[t], idx[t] % G, idx[t] // G
            second[k], second_sub[k] = others[t].min(), same[t].min()
    return sep2, partner, substep, second, second_sub


def sampled_gap(plans, S, pairs, r, z, samples=1001):
    """For the (a, b) pairs given, per (pair, sub-step): the closed-form minimum, the minimum over `samples` equally spaced t,
    |e|^2_w, and the rounding slack of one evaluation of q (1e-12 of |d0|^2_w + |e|^2_w: a few thousand ulp of its largest term)."""
    plans = np.asarray(plans, np.float64)
    P = plans[:, :S + 1, :3]
    a, b = pairs[:, 0], pairs[:, 1]
    d0 = P[a, :S] - P[b, :S]
    e = (P[a, 1:S + 1] - P[b, 1:S + 1]) - d0                                # [m][S][3]
    ee, de = wdot(e, e, r, z), wdot(d0, e, r, z)
    t = np.where(ee > 0, np.clip(-de / np.where(ee > 0, ee, 1.0), 0.0, 1.0), 0.0)
    dc = np.where((t >= 1.0)[..., None], P[a, 1:S + 1] - P[b, 1:S + 1], d0 + t[..., None] * e)
    closed = wdot(dc, dc, r, z)
    ts = np.linspace(0.0, 1.0, samples)
    d = d0[:, :, None, :] + ts[None, None, :, None] * e[:, :, None, :]
    sampled = wdot(d, d, r, z).min(axis=2)
    return closed, sampled, ee, 1e-12 * (wdot(d0, d0, r, z) + ee)


def np_track(plans, has, S, first, n_local, world, worigin, vs, raycast):
    """occupied, unknown, crossed, pot, dist, speed per subject: voxel look-ups under P[s + 1] and the Python Raycast over the
    world grid from P[s] to P[s + 1] (limit: the segment's length in voxels), every occupied value read as 100."""
    plans = np.asarray(plans, np.float64)
    out = {k: np.zeros(n_local, np.int64) for k in ("occupied", "unknown", "crossed", "pot")}
    out["dist"], out["speed"] = np.zeros(n_local), np.zeros(n_local)
    if world is not None:
        wz, wy, wx = world.shape
        val = lambda i, j, k: min(int(world[k, j, i]), 100)
    for k in range(n_local):
        a = first + k
        if not has[a]:
            continue
        p = plans[a, :S + 1, :3]
        v = plans[a, S, 3:6]
        out["speed"][k] = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        for s in range(S):
            d = p[s + 1] - p[s]
            out["dist"][k] += math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if world is None:
                continue
            l0 = [(p[s][c] - worigin[c]) / vs for c in range(3)]
            l1 = [(p[s + 1][c] - worigin[c]) / vs for c in range(3)]
            i, j, kk = (int(math.floor(x)) for x in l1)
            if 0 <= i < wx and 0 <= j < wy and 0 <= kk < wz:
                w = int(world[kk, j, i])
                if w >= 100:
                    out["occupied"][k] += 1
                elif w < 0:
                    out["unknown"][k] += 1
                else:
                    out["pot"][k] += w
            dl = [l0[c] - l1[c] for c in range(3)]
            _, hit = raycast(val, (wx, wy, wz), l0, l1, math.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]))
            if hit is not None:
                out["crossed"][k] += 1
    return out


class Flight:
    """The flight record of n_local agents accumulated in plain Python from per-round results (the restatement of
    hdsm_flight_report): feed it sep2 / partner / substep and the track dict of every round."""

    def __init__(self, n_local, S, sep_warn=1.0):
        self.S, self.warn2 = S, sep_warn * sep_warn
        z = lambda dt=np.int64: np.zeros(n_local, dt)
        self.rounds, self.positions, self.close_rounds = z(), z(), z()
        self.sep2_min, self.sep_partner, self.sep_substep, self.sep_round = np.full(n_local, BIG), np.full(n_local, -1), z(), np.full(n_local, -1)
        self.occupied, self.unknown, self.crossed, self.pot_sum = z(), z(), z(), z()
        self.dist, self.speed_sum, self.speed_max = z(float), z(float), z(float)

    def add(self, has_local, sep2, partner, substep, track):
        for k in np.nonzero(np.asarray(has_local))[0]:
            if sep2[k] < self.sep2_min[k]:
                self.sep2_min[k], self.sep_partner[k], self.sep_substep[k], self.sep_round[k] = sep2[k], partner[k], substep[k], self.rounds[k]
            if sep2[k] < self.warn2:
                self.close_rounds[k] += 1
            for f, g in (("occupied", "occupied"), ("unknown", "unknown"), ("crossed", "crossed"), ("pot_sum", "pot")):
                getattr(self, f)[k] += track[g][k]
            self.dist[k] += track["dist"][k]
            self.speed_sum[k] += track["speed"][k]
            self.speed_max[k] = max(self.speed_max[k], track["speed"][k])
            self.rounds[k] += 1
            self.positions[k] += self.S

    def same_as(self, rep, rtol=1e-12):
        """None if the library's report (lib.FLIGHT_REPORT array) equals this record: integers exactly, doubles to rtol."""
        for f in ("rounds", "positions", "sep_partner", "sep_substep", "sep_round", "close_rounds", "occupied", "unknown", "crossed", "pot_sum"):
            if not np.array_equal(rep[f], getattr(self, f)):
                return f, np.nonzero(rep[f] != getattr(self, f))[0][:8]
        for f in ("sep2_min", "dist", "speed_sum", "speed_max"):
            mine = getattr(self, f)
            if not (np.abs(rep[f] - mine) <= rtol * np.abs(mine)).all():
                return f, float(np.abs(rep[f] - mine).max())
        return None


# ---- generators ---------------------------------------------------------------------------------------------------------------
def records(p0, steps, vel=None, n_hor=N_HOR):
    """plans [n][n_hor + 1][9] from start positions p0 [n][3] and per-step displacements steps [n][n_hor][3]."""
    n = p0.shape[0]
    plans = np.zeros((n, n_hor + 1, 9))
    plans[:, 0, :3] = p0
    plans[:, 1:, :3] = p0[:, None, :] + np.cumsum(steps, axis=1)
    plans[:, :, 3:6] = vel if vel is not None else 0.0
    return plans


def random_batch(rng, n=None, step_plan=None, aniso=None):
    """2..200 agents in a box of about 1.2 m per agent^(1/3) moving up to 0.9 m per step: plans, has, step_plan, (r, z)."""
    n = int(np.exp(rng.uniform(np.log(2), np.log(200.999)))) if n is None else n
    S = int(rng.integers(1, 3)) if step_plan is None else step_plan
    side = 1.2 * n ** (1 / 3) + 0.5
    p0 = rng.uniform(0, side, (n, 3))
    steps = rng.uniform(-0.9, 0.9, (n, N_HOR, 3))
    plans = records(p0, steps, vel=rng.uniform(-9, 9, (n, N_HOR + 1, 3)))
    has = (rng.uniform(size=n) < 0.85).astype(np.uint8)
    radii = (0.25, 0.25) if not (rng.uniform() < 0.5 if aniso is None else aniso) else (float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.3, 1.0)))
    return plans, has, S, radii


def crossing_pair():
    """Two agents that swap ends of a 1.5 m segment offset by 0.1 m: >= 1.5 m apart at both round boundaries, 0.1 m apart midway."""
    p0 = np.array([[0.0, 0.0, 1.5], [1.5, 0.1, 1.5]])
    steps = np.zeros((2, N_HOR, 3))
    steps[0, 0], steps[1, 0] = [1.5, 0.0, 0.0], [-1.5, 0.0, 0.0]
    return records(p0, steps), np.ones(2, np.uint8)


def ring(n, radius_sep=1.0, r=0.25, step=0.05):
    """n agents on a ring whose chord is radius_sep * 2 r (the separation limit), each stepping inwards."""
    R = radius_sep * 2 * r / (2 * math.sin(math.pi / n))
    ang = 2 * math.pi * np.arange(n) / n
    p0 = np.stack([R * np.cos(ang), R * np.sin(ang), np.full(n, 1.5)], axis=1)
    steps = np.zeros((n, N_HOR, 3))
    steps[:, :, :2] = -step * p0[:, None, :2] / R
    return records(p0, steps), np.ones(n, np.uint8)


def tracks_in_world(rng, world, worigin, n, vs=0.3, S=2):
    """n records whose first S steps are tracks in / around `world`: random ones, ones that start inside an obstacle, ones that clip
    a pillar between two free end points, ones that leave the world, ones that run along a voxel face."""
    wz, wy, wx = world.shape
    lo, hi = np.asarray(worigin, float), np.asarray(worigin, float) + np.array([wx, wy, wz]) * vs
    occ = np.argwhere(world >= 100)
    p0, steps = np.zeros((n, 3)), rng.uniform(-0.9, 0.9, (n, N_HOR, 3)) * [1, 1, 0.3]
    for t in range(n):
        kind = t % 5
        p0[t] = rng.uniform(lo + 0.5, hi - 0.5)
        if kind == 1 and len(occ):                         # starts inside an obstacle
            c = occ[rng.integers(len(occ))][::-1]
            p0[t] = lo + (c + rng.uniform(0.05, 0.95, 3)) * vs
        elif kind == 2 and len(occ):                       # straight through an occupied voxel, end points a voxel or two outside
            c = lo + (occ[rng.integers(len(occ))][::-1] + 0.5) * vs
            d = rng.normal(size=3) * [1, 1, 0.1]
            d /= np.linalg.norm(d)
            p0[t] = c - d * rng.uniform(0.3, 0.85)
            steps[t, 0] = d * rng.uniform(0.9, 1.7)
        elif kind == 3:                                    # leaves the world
            ax = int(rng.integers(2))
            p0[t, ax] = (hi if rng.uniform() < 0.5 else lo)[ax] + rng.uniform(-0.4, 0.4)
            steps[t, :, ax] = rng.uniform(-0.9, 0.9, N_HOR)
        elif kind == 4:                                    # along a voxel face: one coordinate exactly on a voxel boundary
            ax = int(rng.integers(3))
            p0[t, ax] = lo[ax] + vs * int(rng.integers(1, world.shape[2 - ax] - 1))
            steps[t, :, ax] = 0.0
    return records(p0, steps, vel=rng.uniform(-9, 9, (n, N_HOR + 1, 3))), np.ones(n, np.uint8), S


DBL_MAX = BIG
SEP_RTOL = 1e-12      # sep2 against numpy: the two evaluate the same closed form in a different order of operations
CLEAR = 1e-9          # a partner is compared exactly when numpy's runner-up is more than this (relative) behind


def check_separation(got, plans, has, S, first, n_local, r, z):
    """One batch of the library (host or device form) against the numpy restatement. Returns the number of rows whose runner-up is
    within CLEAR (their partner / sub-step may be the runner-up's). The runner-up of a partner is the best OTHER partner; the
    sub-step is compared where, in addition, the same partner's next best sub-step is either more than CLEAR behind or an exact tie
    (the end of one sub-step and the start of the next are the same positions: both sides then take the smaller sub-step)."""
    sep2, partner, substep, second, second_sub = np_separation(plans, has, S, first, n_local, r, z)
    lone = partner < 0
    assert (got["partner"][lone] == -1).all() and (got["sep2"][lone] == DBL_MAX).all() and (got["substep"][lone] == 0).all()
    assert ((got["partner"] < 0) == lone).all()
    ok = ~lone
    assert (np.abs(got["sep2"][ok] - sep2[ok]) <= SEP_RTOL * sep2[ok]).all(), float(np.abs(got["sep2"][ok] / sep2[ok] - 1).max())
    clear = ok & (second - sep2 > CLEAR * sep2)
    assert (got["partner"][clear] == partner[clear]).all()
    clear_sub = clear & ((second_sub == sep2) | (second_sub - sep2 > CLEAR * sep2))
    assert (got["substep"][clear_sub] == substep[clear_sub]).all()
    return int((ok & ~clear_sub).sum())


def check_track(got, plans, has, S, first, n_local, world, origin, vs=0.3):
    want = np_track(plans, has, S, first, n_local, world, origin, vs, _py_raycast)
    for f in ("occupied", "unknown", "crossed", "pot"):
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8])
    assert np.array_equal(got["dist"], want["dist"]) and np.array_equal(got["speed"], want["speed"])
    return want
