"""Scripted agents on the CPU: hdsm_script_records_host (csrc/script_core.h, the source k_script runs) against the numpy restatement
of tests/script_cases.py, bit for bit, on every case of that file; the argument refusals; the binding and the scenario helpers;
csrc/script_core.h alone under the address and undefined-behaviour sanitizers (tests/script_core_check.cpp: a stand-alone program,
nothing of it is loaded into Python)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import script_cases as scs
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc

CASES = list(scs.cases())
GROUPS = sorted({c[0] for c in CASES}, key=[c[0] for c in CASES].index)


@pytest.mark.parametrize("group", GROUPS)
def test_the_host_form_equals_the_restatement_bit_for_bit(group):
    n = 0
    for name, knots, n_hor, step_plan, dt, predict, rnd in CASES:
        if name != group:
            continue
        got = lib.script_records(knots, n_hor, step_plan, dt, predict, rnd)
        want = scs.expected(name, knots, n_hor, step_plan, dt, predict, rnd)
        assert got.shape == want.shape == (knots.shape[0], n_hor + 1, 9)
        assert got.tobytes() == want.tobytes(), (name, n_hor, step_plan, predict, rnd, float(np.abs(got - want).max()))
        assert (got[:, :, 6:] == 0).all()
        n += 1
    assert n == len(scs.SHAPES) == 72


def test_the_cases_reach_what_they_are_meant_to_reach():
    """The restatement on its own: rest before and behind a track, the right-hand slope on a knot, the two modes apart."""
    sp = scs.special_tracks()
    k, dt = sp["ends-before-round-0"]
    for predict in (0, 1):
        r = scs.records(k, 10, 2, dt, predict, 0)
        assert (r[0, :, :3] == k[0, -1, 1:]).all() and (r[0, :, 3:] == 0).all()
    k, dt = sp["starts-after-the-horizon"]
    r = scs.records(k, 15, 3, dt, 1, 1000)
    assert (r[0, :, :3] == k[0, 0, 1:]).all() and (r[0, :, 3:] == 0).all()
    k, dt = sp["tau-on-the-knots"]
    r = scs.records(k, 10, 1, dt, 0, 7)                    # state i at (7 + i) / 8 s = knot 7 + i exactly
    for i in range(11):
        j = 7 + i
        assert float(7 + i) * dt == k[0, j, 0]
        assert (r[0, i, :3] == k[0, j, 1:]).all()
        assert (r[0, i, 3:6] == (k[0, j + 1, 1:] - k[0, j, 1:]) / (k[0, j + 1, 0] - k[0, j, 0])).all()      # the right-hand segment's
        assert (r[0, i, 3:6] != (k[0, j, 1:] - k[0, j - 1, 1:]) / (k[0, j, 0] - k[0, j - 1, 0])).all()
    k, dt = sp["knots-1e-9-apart"]
    assert k[0, 0, 0] < 3.0 * dt < k[0, 1, 0] and k[0, 1, 0] - k[0, 0, 0] < 1.1e-9
    r = scs.records(k, 7, 1, dt, 0, 0)
    assert abs(r[0, 3, 3]) > 4e8 and (r[0, [2, 4], 3:6] == 0).all() and (r[1, :, 3:6] == 0).all()   # state 3 is ON the first pair
    assert np.isfinite(scs.records(k, 7, 3, dt, 1, 0)).all() and abs(scs.records(k, 7, 3, dt, 1, 0)[0, 7, 0]) > 1e8
    k = scs.random_tracks(64, 164)
    a, b = scs.records(k, 10, 2, 0.1, 0, 1), scs.records(k, 10, 2, 0.1, 1, 1)
    assert (a[:, :3] == b[:, :3]).all() and np.abs(a[:, 3:] - b[:, 3:]).max() > 0.1   # the same up to step_plan, then a straight line
    assert all(len({tuple(v) for v in b[t, 2:, 3:6]}) == 1 for t in range(4))


def test_every_argument_refusal():
    L = lib.load()
    good = np.array([[[0.0, 0, 0, 1], [1.0, 1, 0, 1], [2.5, 1, 1, 1]]])
    out = np.full((1, 11, 9), -7.0)

    def rc(knots, n_script=1, n_knots=None, n_hor=10, step_plan=1, dt=0.1, predict=0, rnd=0, records=out):
        n_knots = knots.shape[1] if n_knots is None else n_knots
        return L.hdsm_script_records_host(n_script, n_knots, knots, n_hor, step_plan, dt, predict, rnd, records)

    assert rc(good) == 0 and not (out == -7.0).any()
    out[:] = -7.0
    same, back, nan_t, inf_p = (good.copy() for _ in range(4))
    same[0, 2, 0], back[0, 1, 0], nan_t[0, 0, 0], inf_p[0, 1, 2] = same[0, 1, 0], -1.0, np.nan, np.inf
    for bad in (same, back, nan_t, inf_p):                                           # times that do not increase, non-finite entries
        assert rc(bad) == lib.HDSM_ERR_BAD_ARG
    assert rc(good, n_knots=0) == lib.HDSM_ERR_BAD_ARG
    assert rc(np.zeros((1, 257, 4)) + np.arange(257)[None, :, None], n_knots=257) == lib.HDSM_ERR_BAD_ARG
    assert rc(np.zeros((1, 256, 4)) + np.arange(256)[None, :, None], n_knots=256) == 0
    out[:] = -7.0
    for kw in (dict(predict=2), dict(predict=-1), dict(n_script=-1), dict(n_hor=0), dict(n_hor=17), dict(step_plan=0), dict(step_plan=11),
               dict(dt=0.0), dict(dt=np.nan), dict(rnd=-1), dict(records=None)):
        assert rc(good, **kw) == lib.HDSM_ERR_BAD_ARG, kw
    assert L.hdsm_script_records_host(1, 3, None, 10, 1, 0.1, 0, 0, out) == lib.HDSM_ERR_BAD_ARG
    assert (out == -7.0).all()                                                       # a refusal writes nothing
    assert L.hdsm_script_records_host(0, 1, None, 10, 1, 0.1, 0, 0, None) == 0       # nobody scripted: nothing to do
    with pytest.raises(lib.HdsmError) as e:
        lib.script_records(back, 10)
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: hdsm_script_records_host"
    with pytest.raises(lib.HdsmError):
        lib.script_records(np.zeros((2, 3)), 10)


def test_the_binding_takes_the_signatures_from_the_header():
    f64, i64 = lib.CTYPES["double*"], lib.CTYPES["int64_t*"]
    want = {"hdsm_dswarm_set_script": [C.c_void_p, C.c_int32, C.c_int32, f64, C.c_int32],
            "hdsm_dswarm_script_stats": [C.c_void_p, i64],
            "hdsm_script_records_host": [C.c_int32, C.c_int32, f64, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int64, f64],
            "hdsm_script_records_batch": [C.c_int32, C.c_int32, C.c_int32, f64, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int64, f64]}
    L = lib.load()
    for name, argtypes in want.items():
        assert name in lib.EXPORTS, name
        restype, got = lib.SIGNATURES[name]
        assert restype is C.c_int and got == argtypes, name
        assert hasattr(L, name)
    assert L.hdsm_dswarm_set_script(None, 0, 1, None, 0) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_dswarm_script_stats(None, np.zeros(3, np.int64)) == lib.HDSM_ERR_BAD_ARG


def test_the_scenario_tracks():
    h = sc.hold_track((1.0, 2.0, 3.0))
    assert h.shape == (1, 4) and h.dtype == np.float64 and h.tolist() == [[0.0, 1.0, 2.0, 3.0]]
    ln = sc.line_track((0.0, 0.0, 1.0), (3.0, 4.0, 1.0), speed=2.0, t0=0.5)
    assert ln.tolist() == [[0.5, 0.0, 0.0, 1.0], [3.0, 3.0, 4.0, 1.0]]
    r = lib.script_records(ln, 10, step_plan=1, dt=0.1, predict=0, round=10)         # tau from 1.0 s: on the way, 2 m/s
    assert r.shape == (1, 11, 9) and np.allclose(np.linalg.norm(r[0, :, 3:6], axis=1), 2.0) and np.allclose(r[0, 0, :3], [0.6, 0.8, 1.0])
    assert (lib.script_records(h, 7, round=1000)[0, :, :3] == [1.0, 2.0, 3.0]).all()
    for bad in (dict(speed=0.0), dict(speed=-1.0)):
        with pytest.raises(ValueError):
            sc.line_track((0, 0, 0), (1, 0, 0), **bad)
    with pytest.raises(ValueError):
        sc.line_track((1, 1, 1), (1, 1, 1), 1.0)


def test_script_core_under_the_sanitizers(tmp_path):
    """Tracks of 1 to 256 knots allocated at exactly their size, states below, on, next to and between the knots and behind the last
    one against a linear scan, records written into exactly (N + 1) x 9 doubles. The program asserts it all itself and must exit 0."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "script_core_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(os.path.dirname(os.path.abspath(__file__)), "script_core_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
