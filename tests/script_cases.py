"""Scripted agents: a numpy restatement of the record a scripted agent publishes, written from the definition in
include/hdsm_swarm.h (not from csrc/script_core.h), and the cases the host form (tests/test_script.py) and k_script
(tests/test_gpu_script.py) are compared with it on, bit for bit.

Definition. A track is n_knots >= 1 knots (t, x, y, z), t strictly increasing. S(tau) = (p, v, a):
    tau <= t_0            p_0, v = a = 0
    tau >= t_last         p_last, v = a = 0
    t_j <= tau < t_{j+1}  w = (p_{j+1} - p_j) / (t_{j+1} - t_j), p = p_j + (tau - t_j) * w, v = w, a = 0
The record of script round q has N + 1 states, state i at tau_i = float(q * step_plan + i) * dt. predict = 0: S(tau_i). predict = 1:
S(tau_i) for i <= step_plan, beyond it p(tau_sp) + (float(i - step_plan) * dt) * v(tau_sp), v(tau_sp), 0.
Every operation below is one IEEE double operation of numpy, in the order written."""
import itertools

import numpy as np

F = np.float64


def track_state(knots, tau):
    """S(tau) as 9 doubles; knots float64 [n_knots][4]"""
    t, p = knots[:, 0], knots[:, 1:4]
    s = np.zeros(9)
    if tau <= t[0]:
        s[:3] = p[0]
        return s
    if tau >= t[-1]:
        s[:3] = p[-1]
        return s
    j = int(np.nonzero(t <= tau)[0][-1])                  # t_j <= tau < t_{j+1}
    assert t[j] <= tau < t[j + 1]
    for c in range(3):
        w = F(p[j + 1, c] - p[j, c]) / F(t[j + 1] - t[j])
        s[c] = p[j, c] + F(tau - t[j]) * w
        s[3 + c] = w
    return s


def records(knots, n_hor, step_plan, dt, predict, rnd):
    """[n_script][n_hor + 1][9] of script round rnd; knots [n_script][n_knots][4]"""
    knots = np.asarray(knots, dtype=F)
    dt = F(dt)
    out = np.zeros((knots.shape[0], n_hor + 1, 9))
    for k in range(knots.shape[0]):
        tau_sp = F(float(rnd * step_plan + step_plan)) * dt
        s_sp = track_state(knots[k], tau_sp)
        for i in range(n_hor + 1):
            if predict == 0 or i <= step_plan:
                out[k, i] = track_state(knots[k], F(float(rnd * step_plan + i)) * dt)
            else:
                ahead = F(float(i - step_plan)) * dt
                for c in range(3):
                    out[k, i, c] = s_sp[c] + ahead * s_sp[3 + c]
                    out[k, i, 3 + c] = s_sp[3 + c]
    return out


def random_tracks(n_knots, seed):
    """Four tracks of n_knots knots: one inside the first seconds (the horizons of rounds 0, 1, 7), a short one inside a horizon, one
    round the times of round 1000 (100 s to 300 s) and one over everything."""
    rng = np.random.default_rng(seed)
    out = np.zeros((4, n_knots, 4))
    for k, (t_lo, t_hi) in enumerate(((-0.3, 3.1), (0.05, 1.2), (90.0, 310.0), (-5.0, 400.0))):
        gaps = rng.uniform(0.2, 1.0, n_knots)
        t = t_lo + (np.cumsum(gaps) - gaps[0]) * ((t_hi - t_lo) / max(float(gaps[1:].sum()), 1.0))
        out[k, :, 0] = t
        out[k, :, 1:3] = rng.uniform(-20.0, 20.0, (n_knots, 2))
        out[k, :, 3] = rng.uniform(0.5, 3.0, n_knots)
    assert (np.diff(out[:, :, 0], axis=1) > 0).all()
    return out


def special_tracks():
    """{name: (knots [n][n_knots][4], dt)} — the edge cases"""
    eighth = np.arange(0, 41) * 0.125                      # knots ON the tau_i of dt = 0.125 (rounds 0, 1, 7 reach 5.25 s)
    rng = np.random.default_rng(5)
    on_knots = np.zeros((2, 41, 4))
    on_knots[:, :, 0] = eighth
    on_knots[:, :, 1:] = rng.uniform(-3.0, 3.0, (2, 41, 3))
    on_knots[1, :, 0] += 125.0                             # ... and on those of round 1000 (tau from 125 s)
    return {
        "ends-before-round-0": (np.array([[[-9.0, 1.0, 2.0, 3.0], [-4.0, 5.0, -1.0, 2.0], [-0.5, 7.0, 7.0, 1.0]]]), 0.1),
        "ends-at-0": (np.array([[[-2.0, 1.0, 2.0, 3.0], [0.0, 5.0, -1.0, 2.0]]]), 0.1),
        "starts-after-the-horizon": (np.array([[[1.0e4, 1.0, 2.0, 3.0], [1.0e4 + 3.0, 5.0, -1.0, 2.0]]]), 0.1),
        "tau-on-the-knots": (on_knots, 0.125),
        # (the first pair brackets tau_3 = 3.0 * 0.1 of round 0: a state ON the nanosecond segment, w of 5e8 m/s)
        "knots-1e-9-apart": (np.array([[[0.3 - 5e-10, 0.0, 0.0, 1.0], [0.3 - 5e-10 + 1e-9, 0.5, -0.25, 1.5]],
                                       [[0.2, 1.0, 1.0, 1.0], [0.2 + 1e-9, 1.0 + 1e-7, 1.0, 1.0]]]), 0.1),
        "coordinates-at-1e4": (np.array([[[-0.13, 1.0e4, -1.0e4, 9.0e3], [0.77, 1.0e4 + 3.3, -1.0e4 + 0.7, 9.0e3 + 1.1]],
                                         [[0.05, 1.0e4, 1.0e4, 1.0e4], [2.9, 1.0e4 - 7.7, 1.0e4 + 2.2, 1.0e4]]]), 0.1),
    }


SHAPES = list(itertools.product((7, 10, 15), (1, 2, 3), (0, 1), (0, 1, 7, 1000)))     # n_hor, step_plan, predict, round


def cases():
    """(name, knots, n_hor, step_plan, dt, predict, round) of every case"""
    tracks = [(f"random-{n}-knots", random_tracks(n, 100 + n), 0.1) for n in (1, 2, 3, 64, 65, 256)]
    tracks += [(name, k, dt) for name, (k, dt) in special_tracks().items()]
    for name, knots, dt in tracks:
        for n_hor, step_plan, predict, rnd in SHAPES:
            yield name, knots, n_hor, step_plan, dt, predict, rnd


_CACHE = {}


def expected(name, knots, n_hor, step_plan, dt, predict, rnd):
    """records() of a case, computed once per process (the CPU and the GPU tests share it)"""
    key = (name, n_hor, step_plan, predict, rnd)
    if key not in _CACHE:
        _CACHE[key] = records(knots, n_hor, step_plan, dt, predict, rnd)
    return _CACHE[key]
