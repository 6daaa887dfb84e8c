"""A vehicle in the loop restated from the text of include/hdsm_swarm.h and the order written at the top of csrc/vehicle_core.h, not
from its code: one IEEE double operation per Python operation (Python floats round every operation to nearest, math.sqrt is correctly
rounded), the yaw's sine and cosine through lib.command_sincos (pinned by tests/test_commands.py), the draws from
tests/tracking_cases.py, the attitude and Eigen's rule from tests/command_cases.py — and the case table the CPU test and the GPU test
share."""
import itertools
import math

import numpy as np

import command_cases as cc
import tracking_cases as tc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc

GZ = -9.81
G3 = (0.0, 0.0, GZ)
N_ROB, RADIUS = 8, 4.0
# What the mirror flight of tests/test_vehicle.py gave on the CPU with the oracle as the solver, recorded before any GPU run
# (tests/test_gpu_vehicle.py asserts the first two against what the device flies): how far the flight leaves its vehicle-less copy (the
# largest difference of a planned position, m), the instances without a solution, and the tracking distance's mean, standard deviation
# and maximum (m).
RECORDED = dict(leaves_by=2.569689, unsolved=14, mean=0.047678, std=0.037373, max=0.218544)


def gusty(**kw):
    """The vehicle of the mirror flight and of the GPU flights: the defaults in a wind of 0.5 m/s^2 along x with gusts of (2, 2, 1) m/s^2."""
    return sc.crazyflie_vehicle(seed=7, wind=(0.5, 0.0, 0.0), gust=(2.0, 2.0, 1.0), **kw)


def scenario():
    return sc.circle_scenario(N_ROB, radius=RADIUS)


def sincos(x):
    s, c = lib.command_sincos(np.array([float(x)]))
    return float(s[0]), float(c[0])


def fields(m):
    v3 = lambda a: [float(x) for x in a]  # noqa: E731
    return dict(n_sub=int(m.n_sub), feed=int(m.feed), acc_from=int(m.acc_from), kp=v3(m.kp), kv=v3(m.kv), k_att=v3(m.k_att),
                tau_rate=float(m.tau_rate), tau_thrust=float(m.tau_thrust), thrust_min=float(m.thrust_min), thrust_max=float(m.thrust_max),
                rate_max=v3(m.rate_max), drag=v3(m.drag), seed=int(m.seed), wind=v3(m.wind), gust=v3(m.gust))


def dot(a, b):
    s = a[0] * b[0] + a[1] * b[1]
    return s + a[2] * b[2]


def clamp(x, lo, hi):
    """(value, clamped)"""
    if x < lo:
        return lo, 1
    if x > hi:
        return hi, 1
    return x, 0


def frame(q):
    x, y, z, w = q
    xx, yy, zz, xy, xz, yz, xw, yw, zw = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
    xb = [1.0 - 2.0 * (yy + zz), 2.0 * (xy + zw), 2.0 * (xz - yw)]
    yb = [2.0 * (xy - zw), 1.0 - 2.0 * (xx + zz), 2.0 * (yz + xw)]
    zb = [2.0 * (xz + yw), 2.0 * (yz - xw), 1.0 - 2.0 * (xx + yy)]
    return xb, yb, zb


def normalise(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) if all(map(math.isfinite, q)) else math.nan
    return [c / n for c in q]


def attitude(acc, sy, cy):
    t = [float(acc[0]) - 0.0, float(acc[1]) - 0.0, float(acc[2]) - GZ]
    tt = dot(t, t)
    zb = [c / math.sqrt(tt) for c in t] if tt > 0 else t
    xi = [cy, sy, 0.0]
    yb = cc.cross(zb, xi)
    xb = cc.cross(yb, zb)
    m = [[xb[r], yb[r], zb[r]] for r in range(3)]
    if not all(math.isfinite(v) for row in m for v in row):
        return [math.nan] * 4
    return list(cc.quaternion(m)[0])


def seat(m, s, yaw):
    """the vehicle (a dict) on the state s [9] and the yaw"""
    f = fields(m) if not isinstance(m, dict) else m
    s = [float(v) for v in s]
    sy, cy = sincos(yaw)
    q = normalise(attitude(s[6:9], sy, cy))
    t = [s[6] - 0.0, s[7] - 0.0, s[8] - GZ]
    tt = dot(t, t)
    thrust = clamp(math.sqrt(tt) if tt >= 0 else math.nan, f["thrust_min"], f["thrust_max"])[0]
    return dict(pos=s[0:3], vel=s[3:6], quat=q, omega=[0.0] * 3, thrust=thrust, yaw_cmd=float(yaw))


def control(f, y, pr, vr, ar, sy, cy):
    """(omega_c, f_c, thrust clamped, a rate clamped)"""
    xb, yb, zb = frame(y["q"])
    ac = []
    for k in range(3):
        a = ar[k] + f["kp"][k] * (pr[k] - y["p"][k])
        a = a + f["kv"][k] * (vr[k] - y["v"][k])
        ac.append(a - G3[k])
    n2 = dot(ac, ac)
    if n2 > 0.0:
        ln = math.sqrt(n2)
        zd = [c / ln for c in ac]
    else:
        zd = list(zb)
    fc, hit_t = clamp(dot(ac, zb), f["thrust_min"], f["thrust_max"])
    yd = cc.cross(zd, [cy, sy, 0.0])
    n2y = dot(yd, yd)
    ny = math.sqrt(n2y) if n2y >= 0 else math.nan
    yd = list(yb) if ny == 0.0 else [c / ny for c in yd]
    xd = cc.cross(yd, zd)
    e = [0.5 * (dot(zd, yb) - dot(yd, zb)), 0.5 * (dot(xd, zb) - dot(zd, xb)), 0.5 * (dot(yd, xb) - dot(xd, yb))]
    oc, hit_r = [], 0
    for k in range(3):
        v, hit = clamp(-(f["k_att"][k] * e[k]), -f["rate_max"][k], f["rate_max"][k])
        oc.append(v)
        hit_r |= hit
    return oc, fc, hit_t, hit_r


def derivative(f, y, oc, fc, w):
    zb = frame(y["q"])[2]
    d = dict(p=list(y["v"]), v=[], o=[], q=[], f=(fc - y["f"]) * (1.0 / f["tau_thrust"]))
    for k in range(3):
        a = y["f"] * zb[k] + G3[k]
        a = a - f["drag"][k] * y["v"][k]
        d["v"].append(a + w[k])
        d["o"].append((oc[k] - y["o"][k]) * (1.0 / f["tau_rate"]))
    q, o = y["q"], y["o"]
    d["q"] = [0.5 * ((q[3] * o[0] + q[1] * o[2]) - q[2] * o[1]),
              0.5 * ((q[3] * o[1] + q[2] * o[0]) - q[0] * o[2]),
              0.5 * ((q[3] * o[2] + q[0] * o[1]) - q[1] * o[0]),
              0.5 * -((q[0] * o[0] + q[1] * o[1]) + q[2] * o[2])]
    return d


def advanced(y, c, k):
    return dict(p=[a + c * b for a, b in zip(y["p"], k["p"])], v=[a + c * b for a, b in zip(y["v"], k["v"])],
                o=[a + c * b for a, b in zip(y["o"], k["o"])], q=[a + c * b for a, b in zip(y["q"], k["q"])], f=y["f"] + c * k["f"])


def rk4(f, y, oc, fc, w, h):
    hh, h6 = 0.5 * h, h / 6.0
    k1 = derivative(f, y, oc, fc, w)
    k2 = derivative(f, advanced(y, hh, k1), oc, fc, w)
    k3 = derivative(f, advanced(y, hh, k2), oc, fc, w)
    k4 = derivative(f, advanced(y, h, k3), oc, fc, w)
    rs = lambda a, b, c, d: ((a + 2.0 * b) + 2.0 * c) + d  # noqa: E731
    out = {}
    for name in ("p", "v", "o", "q"):
        out[name] = [y[name][i] + h6 * rs(k1[name][i], k2[name][i], k3[name][i], k4[name][i]) for i in range(len(y[name]))]
    out["f"] = y["f"] + h6 * rs(k1["f"], k2["f"], k3["f"], k4["f"])
    q = out["q"]
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    n = math.sqrt(n2) if n2 >= 0 else math.nan
    out["q"] = [c / n for c in q]
    return out


def agent_round(m, agent_id, q, step_plan, dt, start, sp, planned_end, vs):
    """One agent's round. sp: step_plan dicts with pos, vel, acc, quat, yaw, valid. Returns (vehicle after, flown [9], d, dvel, pose,
    (flown, reseated, thrust-clamped, rate-clamped))."""
    f = fields(m)
    s = tc.draws(f["seed"], int(agent_id), int(q))
    w = [f["wind"][k] + f["gust"][k] * s[k] for k in range(3)]
    h = float(dt) / float(f["n_sub"])
    y = dict(p=list(vs["pos"]), v=list(vs["vel"]), q=list(vs["quat"]), o=list(vs["omega"]), f=float(vs["thrust"]))
    yaw_cmd = float(vs["yaw_cmd"])
    knot = [float(v) for v in start]
    planned_end = [float(v) for v in planned_end]
    n_t = n_r = 0
    valid = 0
    for j in range(step_plan):
        c = sp[j]
        valid = int(c["valid"])
        zeroed = valid == 0 and all(v == 0.0 for v in c["quat"])
        along = f["feed"] == 1 and valid != 0
        if zeroed:
            p0, v0, a0 = list(y["p"]), [0.0] * 3, [0.0] * 3
        elif along:
            p0, v0, a0 = knot[0:3], knot[3:6], knot[6:9]
        else:
            p0, v0, a0 = list(c["pos"]), list(c["vel"]), list(c["acc"])
        if not zeroed:
            yaw_cmd = float(c["yaw"])
        sy, cy = sincos(yaw_cmd)
        for sub in range(f["n_sub"]):
            if along:
                t = float(sub) * h
                pr = [(p0[k] + v0[k] * t) + 0.5 * (a0[k] * (t * t)) for k in range(3)]
                vr = [v0[k] + a0[k] * t for k in range(3)]
            else:
                pr, vr = p0, v0
            oc, fc, hit_t, hit_r = control(f, y, pr, vr, a0, sy, cy)
            n_t, n_r = n_t + hit_t, n_r + hit_r
            y = rk4(f, y, oc, fc, w, h)
        knot = list(c["pos"]) + list(c["vel"]) + list(c["acc"])
    ok = all(math.isfinite(v) for name in ("p", "v", "o", "q") for v in y[name]) and math.isfinite(y["f"])
    if ok:
        out = dict(pos=y["p"], vel=y["v"], quat=y["q"], omega=y["o"], thrust=y["f"], yaw_cmd=yaw_cmd)
        zb = frame(y["q"])[2]
        acc = []
        for k in range(3):
            a = y["f"] * zb[k] + G3[k]
            a = a - f["drag"][k] * y["v"][k]
            acc.append(a + w[k])
        flown = y["p"] + y["v"] + (acc if f["acc_from"] == 1 else planned_end[6:9])
        d = tc.norm3(*(flown[k] - planned_end[k] for k in range(3)))
        dv = tc.norm3(*(flown[3 + k] - planned_end[3 + k] for k in range(3)))
    else:
        out = seat(f, planned_end, yaw_cmd if math.isfinite(yaw_cmd) else 0.0)
        flown, d, dv = list(planned_end), 0.0, 0.0
    pose = dict(pos=out["pos"], vel=out["vel"], acc=flown[6:9], quat=out["quat"], yaw=out["yaw_cmd"], valid=valid)
    return out, flown, d, dv, pose, (1 if ok else 0, 0 if ok else 1, n_t, n_r)


# ---- between dicts and the library's records ----
def vstate_array(vs_list):
    a = np.zeros(len(vs_list), lib.VEHICLE_STATE)
    for k, v in enumerate(vs_list):
        a["pos"][k], a["vel"][k], a["quat"][k], a["omega"][k] = v["pos"], v["vel"], v["quat"], v["omega"]
        a["thrust"][k], a["yaw_cmd"][k] = v["thrust"], v["yaw_cmd"]
    return a


def vstate_dicts(a):
    return [dict(pos=[float(x) for x in r["pos"]], vel=[float(x) for x in r["vel"]], quat=[float(x) for x in r["quat"]],
                 omega=[float(x) for x in r["omega"]], thrust=float(r["thrust"]), yaw_cmd=float(r["yaw_cmd"])) for r in a]


def command_array(sp_lists):
    """[n][step_plan] dicts -> lib.COMMAND [n][step_plan]"""
    a = np.zeros((len(sp_lists), len(sp_lists[0])), lib.COMMAND)
    for k, row in enumerate(sp_lists):
        for j, c in enumerate(row):
            a["pos"][k, j], a["vel"][k, j], a["acc"][k, j], a["quat"][k, j] = c["pos"], c["vel"], c["acc"], c["quat"]
            a["yaw"][k, j], a["valid"][k, j] = c["yaw"], c["valid"]
    return a


def command_dicts(a):
    return [dict(pos=[float(x) for x in r["pos"]], vel=[float(x) for x in r["vel"]], acc=[float(x) for x in r["acc"]],
                 quat=[float(x) for x in r["quat"]], yaw=float(r["yaw"]), valid=int(r["valid"])) for r in a]


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def same_vehicle(got, want):
    """a lib.VEHICLE_STATE record against a restated vehicle, bit for bit (NaNs: both NaN)"""
    for name in ("pos", "vel", "quat", "omega", "thrust", "yaw_cmd"):
        g, w = np.atleast_1d(np.asarray(got[name], dtype=np.float64)), np.atleast_1d(np.asarray(want[name], dtype=np.float64))
        if not ((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all():
            return False
    return float(got["reserved0"]) == 0.0


def same_pose(got, want):
    if int(got["valid"]) != want["valid"] or int(got["pad"]) != 0 or float(got["reserved0"]) != 0.0:
        return False
    return all(bits(got[name]) == bits(want[name]) for name in ("pos", "vel", "acc", "quat", "yaw"))


# ---- the case table ----
def setpoint(pos, vel=(0.0, 0.0, 0.0), acc=(0.0, 0.0, 0.0), yaw=0.0, valid=1):
    """a command as k_command writes it: the quaternion is the attitude of (acc, yaw); valid 0: the position held"""
    if valid == 0:
        vel = acc = (0.0, 0.0, 0.0)
    sy, cy = sincos(yaw)
    return dict(pos=[float(v) for v in pos], vel=[float(v) for v in vel], acc=[float(v) for v in acc], quat=attitude(acc, sy, cy), yaw=float(yaw),
                valid=int(valid))


ZEROED = dict(pos=[0.0] * 3, vel=[0.0] * 3, acc=[0.0] * 3, quat=[0.0] * 4, yaw=0.0, valid=0)
IDS = (0, 1, 63, 4095, 2 ** 31 - 1)
ROUNDS = (0, 3, 2 ** 40)


def vehicle(**kw):
    return sc.crazyflie_vehicle(**kw)


def _agents(step_plan, rng):
    """one call's agents: (name, start [9], [setpoints], planned_end [9], vehicle dict) — the generic ones and the crafted ones"""
    base = vehicle()
    out = []
    for i in range(3):                                                          # along a plan, the vehicle a little off it
        p = rng.uniform(-5.0, 5.0, 3)
        v, a = rng.uniform(-2.0, 2.0, 3), rng.uniform(-3.0, 3.0, 3)
        yaw = float(rng.uniform(-3.0, 3.0))
        start = np.concatenate([p, v, a])
        sps, x = [], start.copy()
        for j in range(step_plan):
            x = np.concatenate([x[:3] + 0.1 * x[3:6] + 0.005 * x[6:9], x[3:6] + 0.1 * x[6:9], x[6:9] + rng.uniform(-0.5, 0.5, 3)])
            sps.append(setpoint(x[:3], x[3:6], x[6:9], yaw, 1 + (i == 2)))
        vs = seat(base, start + np.concatenate([rng.uniform(-0.05, 0.05, 6), np.zeros(3)]), yaw + 0.1)
        vs["omega"] = [float(v) for v in rng.uniform(-0.5, 0.5, 3)]
        out.append((f"generic{i}", start, sps, x.copy(), vs))
    rest = np.array([1.0, -2.0, 1.5, 0, 0, 0, 0, 0, 0.0])
    at_rest = seat(base, rest, 0.3)
    far = rest.copy()
    far[:3] += (0.0, 60.0, 5.0)                                                 # thrust and rates into their clamps
    out.append(("clamps", far, [setpoint(far[:3], yaw=0.3)] * step_plan, far, dict(at_rest)))
    fall = setpoint(rest[:3], acc=(0.0, 0.0, GZ))                               # a_c = 0 exactly: z_d = z_b, and y_d from it
    out.append(("a_c-zero", rest, [fall] * step_plan, rest, dict(at_rest, yaw_cmd=0.0)))
    side = setpoint(rest[:3], acc=(5.0, 0.0, GZ), yaw=0.0)                      # a_c along x_i: z_d x x_i = 0, the zero-norm branch
    out.append(("zd-parallel-xi", rest, [side] * step_plan, rest, seat(base, rest, 0.0)))
    out.append(("zeroed", rest, [dict(ZEROED)] * step_plan, rest, dict(at_rest)))
    out.append(("no-plan-hold", rest, [setpoint(rest[:3], valid=0, yaw=0.3)] * step_plan, rest, dict(at_rest)))
    bad = rest.copy()
    bad[4] = np.nan                                                             # one start state that is not finite
    out.append(("not-finite-start", bad, [setpoint(rest[:3] + 0.1, yaw=0.3)] * step_plan, rest + 0.01, dict(at_rest)))
    return out


def cases():
    """(name, model, ids [n], q, step_plan, dt, start [n][9], setpoints [n][step_plan] of dicts, planned_end [n][9], vehicles [n] of dicts)"""
    rng = np.random.default_rng(20261021)
    for n_sub, step_plan, feed, acc_from in itertools.product((1, 2, 10), (1, 3), (0, 1), (0, 1)):
        k = (n_sub + step_plan + feed + acc_from) % len(ROUNDS)
        m = vehicle(n_sub=n_sub, feed=feed, acc_from=acc_from, seed=11 + n_sub, wind=(0.3, -0.2, 0.1), gust=(1.0, 1.5, 0.5))
        ag = _agents(step_plan, rng)
        ids = np.array([IDS[(i + k) % len(IDS)] for i in range(len(ag))], dtype=np.int32)
        yield (f"sub{n_sub}-step{step_plan}-feed{feed}-acc{acc_from}", m, ids, ROUNDS[k], step_plan, 0.1, np.array([a[1] for a in ag]),
               [a[2] for a in ag], np.array([a[3] for a in ag]), [a[4] for a in ag], [a[0] for a in ag])


N_CASES = 24
