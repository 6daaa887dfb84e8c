"""Commands for the vehicle restated from the text of include/hdsm_swarm.h, not from csrc/command_core.h: the yaw step, the attitude
and Eigen's matrix-to-quaternion rule in Python floats with math.atan2 / math.cos / math.sin, and the samples, crafted cases and
batches the CPU test and the GPU test share.

E is the measured maximum absolute error of the library's own atan2 and sincos against numpy.longdouble on the fixed sample of
atan2_sample() / sincos_sample() (atan2 4.33e-16 — an ulp of pi is 4.4e-16 — sin 1.57e-16, cos 1.72e-16). The tests
assert 2 E on that sample; E itself has to stay below 1e-12, the agreement asked of a device flight against its mirror."""
import math

import numpy as np

E = 4.33e-16
assert E < 1e-12
G = 9.81


def tol(want):
    """4 E plus 8 ulp of the compared value"""
    return 4 * E + 8 * np.spacing(np.abs(np.asarray(want, dtype=np.float64)))


# ---- the samples of the accuracy test ----
def atan2_sample():
    """(y, x): a 257 x 257 grid over [-4, 4]^2, 20 000 seeded pairs over the magnitudes 1e-300 .. 1e300, both axes, +-0, and arguments
    within 1e-12 of the cut at +-pi. The pair (0, 0) of the grid is left to the special cases."""
    g = np.linspace(-4.0, 4.0, 257)
    gy, gx = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    rng = np.random.default_rng(20261021)
    ry = rng.choice([-1.0, 1.0], 20000) * 10.0 ** rng.uniform(-300, 300, 20000)
    rx = rng.choice([-1.0, 1.0], 20000) * 10.0 ** rng.uniform(-300, 300, 20000)
    mags = np.array([1e-300, 1e-12, 0.3, 1.0, 7.0, 1e12, 1e300])
    ay = np.concatenate([mags, -mags, np.zeros(14), -np.zeros(14)])
    ax = np.concatenate([np.zeros(7), -np.zeros(7), mags, -mags, mags, -mags])
    cut = np.array([1e-12, 1e-13, 1e-15, 1e-16, 1e-300, 5e-324])
    cy = np.concatenate([cut, -cut, 3.0 * cut, -3.0 * cut])
    cx = np.concatenate([-np.ones(12), -3.0 * np.ones(12)])
    y, x = np.concatenate([gy, ry, ay, cy]), np.concatenate([gx, rx, ax, cx])
    keep = ~((y == 0) & (x == 0))
    return np.ascontiguousarray(y[keep]), np.ascontiguousarray(x[keep])


def sincos_sample():
    """20 000 seeded points of [-1e4, 1e4] and every multiple of pi / 2 in that range with its two neighbours"""
    rng = np.random.default_rng(20261022)
    k = np.arange(-6366, 6367) * (np.pi / 2)
    return np.concatenate([rng.uniform(-1e4, 1e4, 20000), k, np.nextafter(k, -np.inf), np.nextafter(k, np.inf), [1e4, -1e4]])


SPECIAL = [(y, x) for y in (0.0, -0.0, 1.0, -1.0, 2.5e-310, -7e300, math.inf, -math.inf) for x in (0.0, -0.0, 1.0, -1.0, 3e-320, -4e299, math.inf, -math.inf)]


# ---- the restatement ----
def finite(*v):
    return all(math.isfinite(float(x)) for x in v)


def yaw_step(yaw, n_ref, yaw_idx, ref, state, k_p, dt):
    """(yaw after, stepped)"""
    if not n_ref > yaw_idx:
        return yaw, False
    v = [float(ref[c]) - float(state[c]) for c in range(3)]
    if not finite(*v):
        return yaw, False
    if not (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > 0.1:
        return yaw, False
    err = math.atan2(v[1], v[0]) - yaw
    if err > math.pi:
        err = err - 2 * math.pi
    elif err < -math.pi:
        err = err + 2 * math.pi
    return yaw + k_p * err * dt, True


def quaternion(m):
    """Eigen's rule on a 3 x 3 list of lists: ((x, y, z, w), branch) with branch 'T' or the leading index 0, 1, 2"""
    T = m[0][0] + m[1][1] + m[2][2]
    if T > 0:
        s = math.sqrt(T + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        return ((m[2][1] - m[1][2]) * s, (m[0][2] - m[2][0]) * s, (m[1][0] - m[0][1]) * s, w), "T"
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    s = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    q = [0.0, 0.0, 0.0]
    q[i] = 0.5 * s
    s = 0.5 / s
    w = (m[k][j] - m[j][k]) * s
    q[j] = (m[j][i] + m[i][j]) * s
    q[k] = (m[k][i] + m[i][k]) * s
    return (q[0], q[1], q[2], w), i


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def attitude(acc, yaw):
    t = [float(acc[0]), float(acc[1]), float(acc[2]) + G]
    tt = t[0] * t[0] + t[1] * t[1] + t[2] * t[2]
    zb = [c / math.sqrt(tt) for c in t] if tt > 0 else t
    xi = [math.cos(yaw), math.sin(yaw), 0.0]
    yb = cross(zb, xi)
    xb = cross(yb, zb)
    return quaternion([[xb[r], yb[r], zb[r]] for r in range(3)])


ZERO = dict(pos=[0.0] * 3, vel=[0.0] * 3, acc=[0.0] * 3, quat=[0.0] * 4, yaw=0.0, valid=0, branch=None)


def command(s, yaw, valid):
    s = [float(x) for x in s]
    if not finite(*s, yaw):
        return dict(ZERO)
    x = s if valid else s[:3] + [0.0] * 6
    q, branch = attitude(x[6:9], yaw)
    if not finite(*q):
        return dict(ZERO)
    return dict(pos=x[0:3], vel=x[3:6], acc=x[6:9], quat=list(q), yaw=yaw, valid=int(valid), branch=branch)


def agent_round(yaw, n_ref, ref, before, record, valid, after, step_plan, dt, yaw_idx, k_p):
    """(yaw after, stepped, [setpoint commands], pose command) of one agent"""
    yaw, stepped = yaw_step(float(yaw), int(n_ref), yaw_idx, ref, before, k_p, dt)
    sp = [command(record[j + 1] if valid else after, yaw, valid) for j in range(step_plan)]
    return yaw, stepped, sp, command(after, yaw, valid)


def close(got, want):
    """a lib.COMMAND record against a restated command: valid equal, every field within tol"""
    if int(got["valid"]) != want["valid"]:
        return False
    for name in ("pos", "vel", "acc", "quat"):
        if not (np.abs(np.asarray(got[name]) - np.asarray(want[name])) <= tol(want[name])).all():
            return False
    return bool(abs(float(got["yaw"]) - want["yaw"]) <= tol(want["yaw"]))


# ---- crafted agents: every branch of the yaw step, of the attitude and of the record ----
def _tenth():
    """x with fl(x * x) == 0.1 exactly, and its neighbours on either side of the 0.1 rule"""
    x = math.sqrt(0.1)
    for _ in range(8):
        if x * x == 0.1:
            break
        x = math.nextafter(x, math.inf if x * x < 0.1 else -math.inf)
    assert x * x == 0.1
    lo, hi = x, x
    while lo * lo >= 0.1:
        lo = math.nextafter(lo, -math.inf)
    while hi * hi <= 0.1:
        hi = math.nextafter(hi, math.inf)
    return lo, x, hi


ACCS = [(0.0, 0.0, -20.0), (15.0, 0.0, -9.81), (0.0, 15.0, -9.81), (0.0, 0.0, -9.81), (0.0, 0.0, 0.0), (1.0, -2.0, 3.0), (0.0, 0.0, 4.0)]
YAWS = [0.0, math.pi / 2, 3.0, -2.5]


def crafted(n_hor=10, yaw_idx=3):
    """A dict of arrays as lib.command takes them, one crafted agent per row, and the row names"""
    rows, names = [], []
    base = dict(yaw=0.0, n_ref=n_hor + 1, ref=(2.0, 1.0, 0.5), before=np.zeros(9), valid=1, acc=(0.5, -0.5, 1.0), after=None, knot_nan=False)

    def add(name, **kw):
        rows.append(dict(base, **kw))
        names.append(name)

    for a in ACCS:                                     # the T > 0 branch, each leading index, the zero thrust vector
        for y in YAWS:
            add(f"acc{a}-yaw{y:.3g}", acc=a, yaw=y, ref=(0.1, 0.0, 0.0))     # (the reference point too close: the yaw stays what it is)
    lo, x, hi = _tenth()
    for name, v in (("below-0.1", lo), ("at-0.1", x), ("above-0.1", hi)):
        add(name, ref=(v, 0.0, 0.0), yaw=0.7)
    add("n_ref-equals-yaw_idx", n_ref=yaw_idx, yaw=0.4)
    add("n_ref-zero", n_ref=0, yaw=-0.4)
    add("wrap-down", yaw=3.0, ref=(2 * math.cos(-3.0), 2 * math.sin(-3.0), 0.0))
    add("wrap-up", yaw=-3.0, ref=(2 * math.cos(3.0), 2 * math.sin(3.0), 0.0))
    add("behind", yaw=0.0, ref=(-3.0, -0.0, 0.0))
    add("before-nan", before=np.array([np.nan] + [0.0] * 8), yaw=0.3)
    add("before-inf", before=np.array([0.0, np.inf] + [0.0] * 7), yaw=0.3)
    add("after-inf", after=np.array([1.0, 2.0, 3.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0]))
    add("after-nan-acc", after=np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, np.nan, 0.0]))
    add("knot-nan", knot_nan=True)
    add("fallback", valid=2, yaw=1.0)
    add("no-plan", valid=0, yaw=-1.0)
    add("no-plan-far", valid=0, yaw=2.0, ref=(-5.0, 5.0, 0.0))
    add("large-yaw", yaw=9999.5, ref=(1.0, 1.0, 0.0))
    n = len(rows)
    rng = np.random.default_rng(5)
    out = dict(yaw=np.zeros(n), n_ref=np.zeros(n, np.int32), ref_point=np.zeros((n, 3)), state_before=np.zeros((n, 9)),
               records=np.zeros((n, n_hor + 1, 9)), valid=np.zeros(n, np.int32), state_after=np.zeros((n, 9)))
    for k, r in enumerate(rows):
        out["yaw"][k], out["n_ref"][k], out["ref_point"][k], out["state_before"][k], out["valid"][k] = r["yaw"], r["n_ref"], r["ref"], r["before"], r["valid"]
        rec = rng.uniform(-3.0, 3.0, (n_hor + 1, 9))
        rec[:, 6:9] = r["acc"]                         # every knot carries the crafted acceleration ...
        if r["knot_nan"]:
            rec[2, 4] = np.nan
        out["records"][k] = rec
        out["state_after"][k] = rec[1] if r["after"] is None else r["after"]
        if r["after"] is None:
            out["state_after"][k, 6:9] = r["acc"]      # ... and so does the state the round ends in
    return out, names


def batch(n, n_hor=10, seed=0):
    """n agents: the crafted rows first (as many as fit), seeded random agents behind them"""
    c, _ = crafted(n_hor)
    m = len(c["yaw"])
    rng = np.random.default_rng(1000 + seed)
    out = dict(yaw=rng.uniform(-7.0, 7.0, n), n_ref=np.full(n, n_hor + 1, np.int32), ref_point=rng.uniform(-4.0, 4.0, (n, 3)),
               state_before=rng.uniform(-4.0, 4.0, (n, 9)), records=rng.uniform(-6.0, 6.0, (n, n_hor + 1, 9)),
               valid=rng.integers(0, 3, n).astype(np.int32), state_after=rng.uniform(-6.0, 6.0, (n, 9)))
    for key, v in c.items():
        out[key][:min(n, m)] = v[:n]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ---- the flight of the mirror test: the 8-agent exchange on a circle of 4 m, turned by a seeded angle ----
N_FLIGHT, ROUNDS_FLIGHT, RADIUS, SEED = 8, 30, 4.0, 3


def exchange(seed=SEED, n=N_FLIGHT, radius=RADIUS, cx=18.0, cy=15.0, z=1.5):
    """circle_scenario's exchange with the circle turned by a seeded angle: on the unturned circle agent 0 looks along -x from yaw 0,
    an error of exactly pi, where the last bit of atan2 decides which way the wrap goes"""
    phi = float(np.random.default_rng(seed).uniform(0.05, 0.7))
    ang = 2 * np.pi * np.arange(n) / n + phi
    starts = np.stack([cx + radius * np.cos(ang), cy + radius * np.sin(ang), np.full(n, z)], axis=1)
    return starts, starts[(np.arange(n) + n // 2) % n].copy()
