"""Stale plans on the CPU: hdsm_link_deliver_host (csrc/link_core.h, the source k_deliver runs) against the independent rendering of
tests/link_cases.py over crafted and random fate tables; the same header under the address and undefined-behaviour sanitizers
(tests/link_core_check.cpp: a stand-alone program, nothing of it is loaded into Python); the new entry points as the binding reads
them from the headers; scenarios.link_table. What the solver and the device loop do with a shift is tested on the GPU
(tests/test_gpu_plan_shift.py, tests/test_gpu_links.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import link_cases as lc
from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd import scenarios as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def _fly(fate, n_slots, n_hor, step_plan, time_aware, rounds, seed):
    rng = np.random.default_rng(seed)
    plans0, has0 = lc.random_records(rng, n_slots, n_hor, absent=0.0), np.ones(n_slots, np.uint8)
    got = lib.LinkView(fate, n_slots, n_hor, step_plan, time_aware, plans0, has0)
    want = lc.PyLinkView(fate, n_slots, n_hor, step_plan, time_aware, plans0, has0)
    assert got.max_delay == want.D
    for r in range(rounds):
        truth = lc.random_records(rng, n_slots, n_hor)
        got.deliver(truth), want.deliver(truth)
        lc.same_view(got, want)
        assert got.ring[r % (got.max_delay + 1)].tobytes() == truth.tobytes()     # the round's records are in the ring
    return got


@pytest.mark.parametrize("name", list(lc.crafted_tables(5)))
@pytest.mark.parametrize("time_aware", [True, False], ids=["time-aware", "as-is"])
def test_deliver_host_on_the_crafted_tables(name, time_aware):
    fate = lc.crafted_tables(5)[name]
    v = _fly(fate, 6, 10, 3, time_aware, 2 * fate.shape[0] + 9, seed=len(name))       # (6 slots: one of padding, delivered on time)
    assert v.seen_round[5] == v.round - 1 and v.shift[5] == 0 and v.counters[5, 1] == 0
    if name == "all-lost":
        assert (v.seen_round[:5] == -1).all() and (v.counters[:5, 0] == 0).all() and (v.counters[:5, 2] == v.round).all()
        assert (v.shift[:5] == (10 if time_aware else 0)).all()
    if name == "dark-longer-than-ring":
        assert v.counters[2, 2] == 10 and v.counters[2, 1] >= 9 and (v.counters[[0, 1, 3, 4], 2] == 1).all()
    if name == "delay-7":
        assert v.max_delay == 7 and v.counters[0, 2] == 7 and v.counters[0, 0] == v.round - 7


def test_an_older_record_that_arrives_after_a_newer_one_is_ignored():
    fate = lc.crafted_tables(3)["out-of-order"]
    rng = np.random.default_rng(0)
    v = lib.LinkView(fate, 3, 7, 1, True, lc.random_records(rng, 3, 7, 0.0), np.ones(3, np.uint8))
    rounds, truths = [], []
    for r in range(6):
        truths.append(lc.random_records(rng, 3, 7, 0.0))
        v.deliver(truths[-1])
        rounds.append(v.seen_round.copy())
    assert [int(x[0]) for x in rounds] == [-1, 1, 2, 3, 4, 5]           # round 0's record, 3 late, never shows: round 1's came first
    assert [int(x[1]) for x in rounds] == [0, 1, 1, 1, 3, 5]            # rounds 2 and 3 land together in round 4: the newer one
    assert v.counters[0].tolist() == [5, 0, 1, 6] and v.counters[1].tolist() == [4, 1, 2, 6]
    assert v.seen[1].tobytes() == truths[5][1].tobytes()


@pytest.mark.parametrize("seed", range(8))
def test_deliver_host_on_random_tables(seed):
    rng = np.random.default_rng(100 + seed)
    n_rob, pad, n_rounds, n_hor = int(rng.integers(1, 12)), int(rng.integers(0, 3)), int(rng.integers(1, 13)), int(rng.integers(1, 17))
    fate = lc.random_table(rng, n_rounds, n_rob, loss=float(rng.choice([0.0, 0.1, 0.5])), dmax=int(rng.integers(0, 8)))
    _fly(fate, n_rob + pad, n_hor, int(rng.integers(1, 4)), bool(seed & 1), 2 * n_rounds + 9, seed)


def test_deliver_host_refuses_bad_arguments():
    fate = np.zeros((2, 2), np.int8)
    v = lib.LinkView(fate, 2, 4, 1, True, np.zeros((2, 5, 9)), np.ones(2, np.uint8))
    v.deliver(np.zeros((2, 5, 9)))
    v.round = 0                                            # the view already holds round 0
    with pytest.raises(lib.HdsmError) as e:
        v.deliver(np.zeros((2, 5, 9)))
    assert e.value.code == lib.HDSM_ERR_BAD_ARG
    v.round, v.fate = 1, np.full((2, 2), 3, np.int8)       # a delay longer than the ring the view was made for
    with pytest.raises(lib.HdsmError):
        v.deliver(np.zeros((2, 5, 9)))
    L = lib.load()
    assert L.hdsm_link_deliver_host(1, 1, 4, 1, 1, None, 0, 1, 0, None, None, None, None, None, None, None) == lib.HDSM_ERR_BAD_ARG


def test_the_new_entry_points_are_exported_with_their_argument_types():
    L = lib.load()
    f64, i32, i8, u8, i64 = (np.dtype(t) for t in (np.float64, np.int32, np.int8, np.uint8, np.int64))
    want = {"hdsm_set_plan_shift": [C.c_void_p, C.c_int32, i32],
            "hdsm_set_plan_shift_device": [C.c_void_p, i32],
            "hdsm_set_own_plans_device": [C.c_void_p, f64, u8],
            "hdsm_dswarm_set_links": [C.c_void_p, C.c_int32, i8, C.c_int32],
            "hdsm_dswarm_link_stats": [C.c_void_p, i64],
            "hdsm_dswarm_download_seen": [C.c_void_p, f64, u8, i32, i32],
            "hdsm_link_deliver_host": [C.c_int32] * 5 + [i8] + [C.c_int32] * 3 + [f64, f64, f64, u8, i32, i32, i32]}
    for name, args in want.items():
        assert name in lib.EXPORTS, name
        restype, argtypes = lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(args), name
        for got, exp in zip(argtypes, args):
            assert (got.dtype == exp) if isinstance(exp, np.dtype) else (got is exp), (name, got, exp)
        assert hasattr(L, name) and list(getattr(L, name).argtypes) == list(argtypes)
    assert L.hdsm_version() == (1 << 16) | 9               # the features are discovered by symbol: the version word stays
    assert lib.LINK_MAX_DELAY == 7
    # null handles are refused before any device is touched
    assert L.hdsm_set_plan_shift(None, 0, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_set_plan_shift_device(None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_set_own_plans_device(None, None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_dswarm_set_links(None, 0, None, 0) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_dswarm_link_stats(None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_dswarm_download_seen(None, None, None, None, None) == lib.HDSM_ERR_BAD_ARG


def test_link_table():
    t = sc.link_table(40, 9, loss=0.25, delay_min=1, delay_max=3, seed=5, dark=[(4, 3, 8), (0, 39, 39)])
    assert t.dtype == np.int8 and t.shape == (40, 9) and t.tobytes() == sc.link_table(40, 9, 0.25, 1, 3, 5, dark=[(4, 3, 8), (0, 39, 39)]).tobytes()
    assert set(np.unique(t)) <= {-1, 1, 2, 3} and (t[3:9, 4] == -1).all() and t[39, 0] == -1
    lost = (t == -1).mean()
    assert 0.15 < lost < 0.40, lost                        # 360 draws at 0.25 (+ 7 dark cells): 0.25 +- 4 sigma = 0.16 .. 0.34
    assert (sc.link_table(5, 3) == 0).all() and (sc.link_table(5, 3, loss=1.0) == -1).all()
    assert (sc.link_table(6, 2, delay_min=7, delay_max=7) == 7).all()
    for bad in (dict(delay_max=8), dict(delay_min=2, delay_max=1), dict(loss=1.5), dict(dark=[(3, 0, 0)]), dict(dark=[(0, 2, 9)])):
        with pytest.raises(ValueError):
            sc.link_table(5, 3, **bad)


def test_link_core_under_the_sanitizers(tmp_path):
    """The step shift for every (N, shift, step), the argument checks, the crafted tables and 60 random flights, every array
    allocated at exactly its size. The program asserts it all itself and must exit 0."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "link_core_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "link_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
