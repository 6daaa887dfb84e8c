"""Missions: the plain-Python restatement of the rule of csrc/mission_core.h (include/hdsm_swarm.h, "missions"), the named cases and
the flights that tests/test_mission.py (host form, host mirror, CPU) and tests/test_gpu_mission.py (k_mission, the device loop) share.
TEST INFRASTRUCTURE, no tests. The restatement shares no source with the library: Python floats are IEEE doubles, every product and
sum is written in the order the header states, math.sqrt is correctly rounded."""
import math

import numpy as np

from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc

DBL_MAX = float(np.finfo(np.float64).max)
R, V, DWELL = 0.3, 0.3, 2          # the thresholds of the flights: 0.3 m, 0.3 m/s, two rounds inside


def _d2(p, w):
    dx, dy, dz = float(p[0]) - float(w[0]), float(p[1]) - float(w[1]), float(p[2]) - float(w[2])
    return (dx * dx + dy * dy) + dz * dz


def _finite(x):
    return x - x == 0.0


def _leg(s, w):
    d2 = _d2(s, w)
    return math.sqrt(d2) if _finite(d2) else DBL_MAX


def blank_records(n):
    """The records hdsm_*_set_mission leaves: zeros, the rounds -1, best_dist DBL_MAX (no distance seen yet)."""
    rec = np.zeros(n, lib.MISSION_RECORD)
    rec["done_round"], rec["last_arrival_round"], rec["arrive_round"], rec["best_dist"] = -1, -1, -1, DBL_MAX
    return rec


def step(setting, records, states, waypoints, count, rnd, goals, due):
    """One step of every agent in mission round rnd, in place on copies: (records, goals, due, summary dict)."""
    rec, goals, due = records.copy(), np.array(goals, dtype=np.float64), np.array(due, dtype=np.uint8)
    Rr, Vv = float(setting.arrive_radius), float(setting.arrive_speed)
    arrivals = 0
    for k in range(len(rec)):
        r, s = rec[k], states[k]
        if r["done"]:
            continue
        w = waypoints[k][int(r["wp"])]
        d2 = _d2(s, w)
        v2 = (float(s[3]) * float(s[3]) + float(s[4]) * float(s[4])) + float(s[5]) * float(s[5])
        finite = _finite(d2) and _finite(v2)
        d = math.sqrt(d2) if finite else -1.0
        inside = finite and d2 <= Rr * Rr and (Vv <= 0.0 or v2 <= Vv * Vv)
        r["dist"] = d
        r["dwell"] = r["dwell"] + 1 if inside else 0
        if r["dwell"] >= setting.dwell_rounds:
            r["arrive_round"][int(r["wp"])] = rnd
            r["last_arrival_round"] = rnd
            r["arrivals"] += 1
            r["wp"] += 1
            r["dwell"] = 0
            if r["wp"] == count[k]:
                if setting.loop:
                    r["wp"] = 0
                    r["laps"] += 1
                else:
                    r["done"], r["done_round"] = 1, rnd
            if not r["done"]:
                nw = waypoints[k][int(r["wp"])]
                goals[k], due[k] = nw, 1
                r["best_dist"], r["since"], r["stalled"] = _leg(s, nw), 0, 0
            arrivals += 1
        elif finite and d < float(r["best_dist"]) - float(setting.stall_eps):
            r["best_dist"], r["since"], r["stalled"] = d, 0, 0
        else:
            r["since"] += 1
            if setting.stall_rounds > 0 and r["since"] == setting.stall_rounds:
                r["stalled"] = 1
                r["stall_events"] += 1
    n, done = len(rec), int(rec["done"].sum())
    summary = dict(round=rnd, flown=n, done=done, stalled=int(((rec["stalled"] != 0) & (rec["done"] == 0)).sum()), arrivals=arrivals,
                   arrivals_total=int(rec["arrivals"].sum()), makespan=int(rec["done_round"].max()) if n and done == n else -1)
    return rec, goals, due, summary


def random_batch(rng, n, n_wp=4, loop=False, stall_rounds=3):
    """A setting, a table and records in the middle of a mission: states scattered round the current waypoint so that about a third
    are inside, some slow and some fast, a few not finite; dwell, since and best_dist anywhere they can be."""
    setting = sc.mission_setting(n_wp, loop=loop, dwell_rounds=2, stall_rounds=stall_rounds, arrive_radius=R, arrive_speed=V, stall_eps=0.05)
    waypoints = rng.uniform(-20.0, 20.0, (n, n_wp, 3))
    count = rng.integers(1, n_wp + 1, n).astype(np.int32)
    rec = blank_records(n)
    rec["wp"] = rng.integers(0, count)
    rec["dwell"] = rng.integers(0, 2, n)
    rec["since"] = rng.integers(0, stall_rounds + 2, n)
    rec["best_dist"] = rng.uniform(0.0, 2.0, n)
    rec["arrivals"] = rec["wp"]
    states = np.zeros((n, 9))
    for k in range(n):
        u = rng.normal(size=3)
        states[k, :3] = waypoints[k, rec["wp"][k]] + u / np.linalg.norm(u) * rng.choice([0.1, 0.29, 0.31, 1.5])
        u = rng.normal(size=3)
        states[k, 3:6] = u / np.linalg.norm(u) * rng.choice([0.0, 0.29, 0.31, 3.0])
    bad = rng.random(n) < 0.05
    states[bad, rng.integers(0, 6, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    done = rng.random(n) < 0.1
    rec["done"][done], rec["done_round"][done] = 1, rng.integers(0, 50, int(done.sum()))
    return setting, rec, states, waypoints, count


def on_the_radius():
    """A position whose squared distance to the origin is EXACTLY R * R in doubles: R along one axis."""
    p = np.array([0.0, R, 0.0])
    assert _d2(p, np.zeros(3)) == R * R
    return p


def named_cases():
    """[(name, setting, records, states, waypoints, count, round)] — one agent each: the edges of the rule."""
    out = []
    wp2 = np.array([[[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]])

    def case(name, setting, state, waypoints=wp2, count=(2,), rnd=7, **fields):
        rec = blank_records(1)
        rec["best_dist"] = 1.0
        for f, v in fields.items():
            rec[f] = v
        s = np.zeros((1, 9))
        s[0, :len(state)] = state
        out.append((name, setting, rec, s, np.asarray(waypoints, dtype=np.float64), np.asarray(count, np.int32), rnd))

    base = dict(dwell_rounds=2, stall_rounds=3, arrive_radius=R, arrive_speed=V, stall_eps=0.05)
    on = on_the_radius()
    case("on the radius, second round inside: arrives", sc.mission_setting(2, **base), on, dwell=1)
    case("just outside the radius", sc.mission_setting(2, **base), on * (1.0 + 2.0 ** -50), dwell=1)
    case("inside but too fast", sc.mission_setting(2, **base), [0.1, 0, 0, 0.31, 0, 0], dwell=1)
    case("inside, fast, no speed test", sc.mission_setting(2, **dict(base, arrive_speed=0.0)), [0.1, 0, 0, 5.0, 0, 0], dwell=1)
    case("speed exactly on the threshold", sc.mission_setting(2, **base), [0.1, 0, 0, 0, V, 0], dwell=1)
    case("one round outside resets the dwell", sc.mission_setting(2, **dict(base, dwell_rounds=3)), [0.5, 0, 0], dwell=2)
    wp16 = np.arange(48, dtype=np.float64).reshape(1, 16, 3)
    case("count 1 of 16: done at once", sc.mission_setting(16, **base), wp16[0, 0], waypoints=wp16, count=(1,), dwell=1)
    case("count 16 of 16: the last waypoint", sc.mission_setting(16, **base), wp16[0, 15], waypoints=wp16, count=(16,), dwell=1, wp=15, arrivals=15)
    case("count 16 of 16, loop: wraps", sc.mission_setting(16, loop=True, **base), wp16[0, 15], waypoints=wp16, count=(16,), dwell=1, wp=15, arrivals=15)
    case("last waypoint without loop: done", sc.mission_setting(2, **base), [3.0, 0, 0], dwell=1, wp=1, arrivals=1)
    case("last waypoint with loop: a lap", sc.mission_setting(2, loop=True, **base), [3.0, 0, 0], dwell=1, wp=1, arrivals=1)
    case("a NaN position", sc.mission_setting(2, **base), [np.nan, 0, 0], dwell=1, since=1)
    case("an infinite velocity", sc.mission_setting(2, **base), [0.1, 0, 0, np.inf, 0, 0], dwell=1, since=1)
    case("stall raised at since == stall_rounds", sc.mission_setting(2, **base), [2.0, 0, 0], since=2)
    case("no stall one round earlier", sc.mission_setting(2, **base), [2.0, 0, 0], since=1)
    case("stall cleared by progress", sc.mission_setting(2, **base), [0.9, 0, 0], since=5, stalled=1, stall_events=1)
    case("progress smaller than stall_eps is none", sc.mission_setting(2, **base), [0.96, 0, 0], since=2)
    case("stall raised again", sc.mission_setting(2, **base), [2.0, 0, 0], since=2, stall_events=1)
    case("stall_rounds 0: never", sc.mission_setting(2, **dict(base, stall_rounds=0)), [2.0, 0, 0], since=2)
    case("done: nothing moves", sc.mission_setting(2, **base), [0.0, 0, 0], dwell=1, done=1, done_round=3, wp=1)
    return out


def assert_same(got, want, tag):
    """(records, goals, due, summary) of a form against the restatement: byte for byte, the summary field by field."""
    assert got[0].tobytes() == want[0].tobytes(), (tag, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (tag, got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes(), (tag, got[2], want[2])
    assert got[3] == want[3], (tag, got[3], want[3])


# ---- the flights ----
FREE_AT = (10.0, 10.0, 1.5)


def shuttle(x0=10.0, y0=10.0, z=1.5):
    """Four agents on lanes 2 m apart, 3 m legs, counts 1, 2, 3, 4: (setting, starts, waypoints, count)."""
    starts, waypoints, _ = sc.shuttle_mission(4, 3.0, 4, x0=x0, y0=y0, z=z)
    return sc.mission_setting(4, arrive_radius=R, arrive_speed=V, dwell_rounds=DWELL), starts, waypoints, np.array([1, 2, 3, 4], np.int32)


def square(loop=False, x0=10.0, y0=10.0, z=1.5):
    """Four agents on the corners of a 3 m square, each visiting the next three corners: (setting, starts, waypoints, count)."""
    starts, waypoints, count = sc.square_mission(3.0, 3, x0=x0, y0=y0, z=z)
    return sc.mission_setting(3, loop=loop, arrive_radius=R, arrive_speed=V, dwell_rounds=DWELL), starts, waypoints, count


def last_waypoints(waypoints, count):
    return np.array([waypoints[k, count[k] - 1] for k in range(len(count))])
