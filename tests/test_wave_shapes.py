"""Every launch shape of the solver kernel through the CPU execution of its device source (tests/wave_emu), against the oracle.

libhdsm.so instantiates hdsm::Solver<NV, CMAX, SMALL> in the eight (kernel, NV, CMAX, threads) shapes of hdsm_shapes.h;
wave_shapes() lists the tuples the emulator runs, the same rows first. The guard below holds them against the kernel symbols of the
built library, and the selection test checks the rule that picks a shape for a launch (hdsm::pick_shape). The capacity tests
fill the staging area of each kernel that shares a CU up to its last row (the answer must be the oracle's, without the overflow flag)
and beyond it (each instance the oracle's answer or HDSM_FLAG_STAGING_OVERFLOW), also with the threads interleaved at every atomic
operation, where the two staging lists claim their slots."""
import os
import re
import shutil

import numpy as np
import pytest

import staging_cases as sc
from kernel_elf import LIB, _kernel_descriptors
from multi_agent_pkgs_amd.params import make_params
from parity_cases import FORCED_SHAPES
from wave_cases import _mixed_batch, compare


@pytest.fixture(scope="module")
def wave():
    from wave_emu import pywave
    pywave.lib()
    return pywave


def _shipped_tuples(tmp_path):
    """{(kernel, NV, CMAX, threads)} of the k_replan* kernels of the built library. Itanium names: <len><name>ILi<NV>ELi<CMAX>ELi<NT>E
    (in hdsm_api.hip's anonymous namespace: _ZN12_GLOBAL__N_1 in front)."""
    out = set()
    for sym in _kernel_descriptors(tmp_path):
        for m in re.finditer(r"(\d+)(k_replan\w*?)ILi(\d+)ELi(\d+)ELi(\d+)E", sym):
            if m.group(1).endswith(str(len(m.group(2)))):   # (_N_1 + 12k_replan_duo reads as "112")
                out.add((m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))))
    return out


def test_every_shipped_kernel_shape_runs_in_the_emulator(wave, tmp_path):
    """Each k_replan* kernel of libhdsm.so has its exact (NV, CMAX, SMALL, threads) tuple in wave_shapes(): a kernel shape added
    to the library without a CPU execution of its source fails here. (Skips exactly when test_no_solver_kernel_uses_scratch does.)"""
    if not os.path.exists(LIB):
        pytest.skip("libhdsm.so not built")
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no ROCm toolchain")
    shipped = _shipped_tuples(tmp_path)
    emulated = {(s["kernel"], s["nv"], s["cmax"], s["threads"]): s for s in wave.wave_shapes()}
    print("shipped kernel shapes:", sorted(shipped))
    assert len(shipped) == 8, sorted(shipped)
    missing = sorted(t for t in shipped if t not in emulated)
    assert not missing, "kernel shapes of libhdsm.so the emulator does not run: %r" % missing
    for t in shipped:   # the small LDS layout belongs to the four-per-CU kernel, and only to it
        assert emulated[t]["small"] == (t[0] == "k_replan_quad"), t
    assert {s["name"] for s in wave.wave_shapes() if s["kernel"] == "-"} >= {"duo48_320"}   # (CPU only: not in the library)


def _create_knobs(n_hor, threads=256, env=None, P=4, RS=18, cus=256):
    """The knobs of hdsm::pick_shape as hdsm_create settles them on an MI355X (256 CUs): HDSM_DUO_MIN (default CUs + 1), then
    HDSM_TRI_MIN (2 x CUs + 1, or 0 when duo_min is 0), then HDSM_QUAD_MIN (3 x CUs + 1, or 0 when tri_min is 0)."""
    env = env or {}
    duo = int(env.get("HDSM_DUO_MIN", cus + 1))
    tri = int(env.get("HDSM_TRI_MIN", 2 * cus + 1 if duo > 0 else 0))
    quad = int(env.get("HDSM_QUAD_MIN", 3 * cus + 1 if tri > 0 else 0))
    return dict(n=3 * n_hor, threads=threads, P=P, RS=RS, duo_min=duo, tri_min=tri, quad_min=quad)


def test_pick_shape_chooses_the_shape_each_pass_launches(wave):
    """hdsm::pick_shape, the one launch rule of hdsm_api.hip, for (ordinary launch or pass 1, pass 2 of a split launch, rescue):
    on the knobs with which test_gpu_parity.py forces each shape on its batch, on the bench line and on cfg 3 and cfg 5."""
    passes = ("ordinary", "items", "rescue")
    forced = {"replan30_64": ("replan30_64", "replan30_64", "replan30_64"), "replan30": ("replan30", "replan30", "replan30"),
              "duo": ("duo", "duo", "replan30"), "tri": ("tri", "duo", "replan30"), "quad": ("quad", "duo", "replan30"),
              "replan48_64": ("replan48_64", "replan48_64", "replan48_64"), "replan48": ("replan48", "replan48", "replan48"),
              "duo48": ("duo48", "duo48", "replan48")}
    assert set(forced) == set(FORCED_SHAPES)
    for shape, (n_hor, threads, env) in FORCED_SHAPES.items():
        knobs = _create_knobs(n_hor, threads, env)
        blocks = 8 if n_hor == 10 else 4   # (test_every_launch_shape_matches_the_oracle: 16 agents, every 2nd / 4th an instance)
        assert tuple(wave.pick_shape(knobs, blocks, p) for p in passes) == forced[shape], (shape, knobs)
    for what, n_inst, n_hor, want in (("bench line", 1024, 10, ("quad", "duo", "replan30")), ("cfg 3", 256, 10, ("replan30", "duo", "replan30")),
                                      ("cfg 5", 4096, 15, ("duo48", "duo48", "replan48"))):
        assert tuple(wave.pick_shape(_create_knobs(n_hor), n_inst, p) for p in passes) == want, what
    # the thresholds at 256 CUs, and the small LDS layout of quad (<= 4 polyhedra of <= 20 rows)
    for blocks, want in ((256, "replan30"), (257, "duo"), (512, "duo"), (513, "tri"), (768, "tri"), (769, "quad")):
        assert wave.pick_shape(_create_knobs(10), blocks) == want, blocks
    assert wave.pick_shape(_create_knobs(10, P=5), 1024) == "tri" and wave.pick_shape(_create_knobs(10, RS=21), 1024) == "tri"
    assert wave.pick_shape(_create_knobs(15), 1024) == "duo48" and wave.pick_shape(_create_knobs(15), 256) == "replan48"


def _shapes(wave, nv):
    return [s["name"] for s in wave.wave_shapes() if s["nv"] == nv and s["cmax"] > 16]


def _orders(wave, name):
    return ("forward", "reverse") if wave.wave_shapes()[[s["name"] for s in wave.wave_shapes()].index(name)]["threads"] > 64 else ("forward",)


def _run(wave, prm, args, shape, order, monkeypatch, yield_atomics=False):
    monkeypatch.setenv("WEMU_ORDER", order)
    if yield_atomics:
        monkeypatch.setenv("WEMU_YIELD_ATOMICS", "1")
    try:
        return wave.replan(prm, *args, shape=shape)
    finally:
        monkeypatch.delenv("WEMU_ORDER")
        monkeypatch.delenv("WEMU_YIELD_ATOMICS", raising=False)


@pytest.mark.parametrize("n_hor,rk4,drag,seed", [(10, False, (0, 0, 0), 310), (12, False, (0, 0, 0), 312), (15, False, (0, 0, 0), 317),
                                                 (15, True, (0.1, 0.1, 0.3), 319)], ids=["h10", "h12", "h15", "h15-rk4-drag"])
def test_every_shape_matches_the_oracle(wave, oracle, monkeypatch, n_hor, rk4, drag, seed):
    """Each shape of its NV (H = 10: NV = 32; H = 12 / 15: NV = 48) on one batch, the multi-wavefront ones in both wave orders."""
    prm = make_params(n_hor=n_hor, rk4=rk4, drag=drag, max_rows_static=18, poly_hor=4)
    args = _mixed_batch(prm, 16, seed, every=2 if n_hor <= 10 else 4)   # (seeds with feasible and infeasible instances)
    o = sc.verdict(oracle, prm, args)
    assert (o["status"] == 0).sum() >= 2 and (o["status"] == 2).sum() + (o["status"] == 0).sum() == len(o["status"])
    for shape in _shapes(wave, 32 if n_hor <= 10 else 48):
        for order in _orders(wave, shape):
            compare(_run(wave, prm, args, shape, order, monkeypatch), o)


@pytest.mark.parametrize("shape", list(sc.CASES))
def test_staging_area_filled_to_just_below_capacity(wave, oracle, monkeypatch, shape):
    """NEAR case of staging_cases: every instance stages between 90 % of the shape's rows and one row less — the oracle's answers,
    no overflow flag, in both wave orders."""
    cmax = sc.CASES[shape]["cmax"]
    prm, args = sc.batch(sc.CASES[shape]["near"])
    o = sc.verdict(oracle, prm, args)
    for order in ("forward", "reverse"):
        e = _run(wave, prm, args, shape, order, monkeypatch)
        print(shape, order, "capacity", cmax, "peak", e["peak"].tolist())
        assert ((e["peak"] >= 0.9 * cmax) & (e["peak"] < cmax)).all(), (cmax, e["peak"].tolist())
        assert (e["flags"] & sc.FLAG_STAGING_OVERFLOW == 0).all()
        compare(e, o)


@pytest.mark.parametrize("mode", ["lockstep", "yield-at-atomics", "two-lists-yield-at-atomics"])
@pytest.mark.parametrize("shape", list(sc.CASES))
def test_staging_overflow_is_exact_or_flagged_at_every_capacity(wave, oracle, monkeypatch, shape, mode):
    """OVER case of staging_cases: sweeps ask for more rows than the shape has. Each instance returns the oracle's answer or carries
    HDSM_FLAG_STAGING_OVERFLOW — never another optimum, never an unflagged NO_SOLUTION for a feasible instance (what the 320-row
    H = 15 kernel did on the GPU in round 6). With yield_atomics (WEMU_YIELD_ATOMICS=1) every thread lets all others run at each
    atomic operation, so the writers of both lists take their increments before any of them reads the other list's counter; the
    emulator audits every sweep (no staging slot with two writers; every slot of a sweep that did not overflow written once).
    The product stages every row into the hot list (hot_tau = 1e30); two-lists sets HDSM_HOT_TAU = 0.1 m, so that rows with more
    slack go to the cold list at the top of the area and the two lists meet when it overflows — where stage_slot's check of the
    other list's counter is what keeps them apart."""
    cmax = sc.CASES[shape]["cmax"]
    prm, args = sc.batch(sc.CASES[shape]["over"])
    o = sc.verdict(oracle, prm, args)
    if mode.startswith("two-lists"):
        monkeypatch.setenv("HDSM_HOT_TAU", "0.1")
    for order in ("forward", "reverse"):
        e = _run(wave, prm, args, shape, order, monkeypatch, mode != "lockstep")
        print(shape, order, "capacity", cmax, "peak", e["peak"].tolist(), "flags", e["flags"].tolist())
        assert (e["peak"] > cmax).sum() >= 2, (cmax, e["peak"].tolist())
        sc.exact_or_flagged(e["status"], e["traj"], e["obj"], e["flags"], o, 1e-8)
        assert (e["cand"] <= cmax).all()


def test_the_320_row_h15_shape_of_round_6_is_exact_or_flagged(wave, oracle, monkeypatch):
    """Solver<48, 320> at 128 threads, the instantiation the library dropped in round 6 after it declared feasible H = 15 instances
    infeasible without the overflow flag on the GPU. Its CPU execution, on the over-capacity H = 15 batch, in both wave orders and
    interleaved at the atomics: every instance the oracle's answer or flagged."""
    prm, args = sc.batch(sc.CASES["duo48"]["over"])
    o = sc.verdict(oracle, prm, args)
    assert (o["status"] == 0).any()
    for order in ("forward", "reverse"):
        for y in (False, True):
            e = _run(wave, prm, args, "duo48_320", order, monkeypatch, y)
            assert (e["peak"] > 320).all()
            sc.exact_or_flagged(e["status"], e["traj"], e["obj"], e["flags"], o, 1e-8)


def test_yield_mode_interleaves_the_slot_claims(wave, monkeypatch):
    """WEMU_YIELD_ATOMICS=1 really changes the schedule at the claims: the same answers, reached with the lanes' atomic operations
    interleaved (the deadlock detector counts a yield as progress), on a one-wavefront and a four-wavefront shape."""
    prm, args = sc.batch(sc.CASES["tri"]["near"])
    for shape in ("replan30_64", "replan30"):
        a = _run(wave, prm, args, shape, "forward", monkeypatch)
        b = _run(wave, prm, args, shape, "forward", monkeypatch, yield_atomics=True)
        assert (a["status"] == b["status"]).all() and (a["peak"] == b["peak"]).all()
        assert np.abs(a["traj"] - b["traj"]).max() < 1e-8
