"""Imperfect tracking on the CPU: hdsm_track_states_host (csrc/track_core.h, the source k_track runs) against the restatement of
tests/tracking_cases.py, bit for bit, on every case of that file; the bound the amplitudes give; the draws' statistics; every
argument refusal; the host mirror flown with the oracle as the solver (SwarmLoop as tests/test_loop_phases.py flies it, 4 agents,
H = 10, 6 rounds): the state after every commit, the next round's solver input, the records, states taken from outside, and a
mirror that never sets a model."""
import ctypes as C

import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
import tracking_cases as tc
from multi_agent_pkgs_amd import lib, swarm
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import Tracking, TrackRecord

CASES = list(tc.cases())
N_FLIGHT, ROUNDS_FLIGHT = 4, 6
MODEL = dict(seed=7, wind=(0.5, 0.0, 0.0), gust=(2.0, 2.0, 1.0), jitter=(0.01, 0.01, 0.005))


@pytest.mark.parametrize("model", [m[0] for m in tc.MODELS])
def test_the_host_form_equals_the_restatement_bit_for_bit(model):
    n = 0
    for name, m, ids, planned, T, q in CASES:
        if not name.startswith(model):
            continue
        flown, dist = lib.track_states(m, ids, planned, T, q)
        want, want_dist = tc.flown_many(m, ids, q, T, planned)
        assert flown.tobytes() == want.tobytes(), (name, float(np.abs(flown - want).max()))
        assert dist.tobytes() == want_dist.tobytes(), name
        assert (flown[:, 6:] == planned[:, 6:]).all()
        dp, dv = tc.bounds(m, T)
        slack = 4 * np.spacing(np.abs(planned[:, :3]).max() + 1.0)          # (the sum p + ... is rounded at the magnitude of p)
        assert (np.abs(flown[:, :3] - planned[:, :3]) <= dp + slack).all(), name
        assert (np.abs(flown[:, 3:6] - planned[:, 3:6]) <= dv + 4 * np.spacing(6.0)).all(), name
        if model == "wind-only":                                             # no draw enters: every agent is pushed the same way
            assert np.abs(flown[:, 3:6] - planned[:, 3:6] - T * np.array(m.wind)).max() < 1e-14
        else:
            assert len({tuple(r) for r in (flown[:, 3:6] - planned[:, 3:6]).round(9)}) == len(ids), name
        n += 1
    assert n == tc.N_CASES // len(tc.MODELS) == 48
    # dist may be NULL
    name, m, ids, planned, T, q = CASES[-1]
    flown = np.zeros_like(planned)
    assert lib.load().hdsm_track_states_host(m, len(ids), ids, planned, T, q, flown, None) == 0
    assert flown.tobytes() == tc.flown_many(m, ids, q, T, planned)[0].tobytes()


def test_the_draws():
    """One seed, ids 0..255 x rounds 0..255 x 6: 393 216 draws of variance 1/3, taken through the library (gust-only and jitter-only
    models at T = 1 and a zero plan make v' = s_ax and p' = s_{3+ax} exactly) and checked against the restatement on a sample."""
    ids = np.arange(256, dtype=np.int32)
    zero = np.zeros((256, 9))
    gust, jit = sc.gust_model(5, gust=(1, 1, 1)), sc.gust_model(5, jitter=(1, 1, 1))
    s = np.zeros((256, 256, 6))
    for q in range(256):
        s[:, q, :3] = lib.track_states(gust, ids, zero, 1.0, q)[0][:, 3:6]
        s[:, q, 3:] = lib.track_states(jit, ids, zero, 1.0, q)[0][:, :3]
    for a, q in ((0, 0), (1, 0), (0, 1), (255, 255), (64, 63)):
        assert s[a, q].tolist() == tc.draws(5, a, q)
    assert (s >= -1.0).all() and (s < 1.0).all()
    flat = s.reshape(-1, 6)
    assert all(len(set(row)) == 6 for row in flat.tolist())                  # no two of the 6 draws of any (id, q) are equal
    assert len(set(flat[:, 0].tolist())) == flat.shape[0]                    # no two (id, q) share their first draw
    n = s.size
    assert n == 393216
    mean, mean_sq = float(s.mean()), float((s * s).mean())
    print(f"{n} draws: mean {mean:+.5f}, mean square {mean_sq:.5f}")
    assert abs(mean) < 0.0046                                                # 5 sigma / sqrt(n), sigma^2 = 1/3
    assert abs(mean_sq - 1.0 / 3.0) < 0.0024                                 # 5 sigma with Var(s^2) = 4/45


def test_every_argument_refusal():
    L = lib.load()
    good = sc.gust_model(**MODEL)
    ids, planned = np.arange(3, dtype=np.int32), np.ones((3, 9))
    flown, dist = np.full((3, 9), -7.0), np.full(3, -7.0)

    def rc(m=good, n=3, ids=ids, planned=planned, T=0.1, rnd=0, flown=flown, dist=dist):
        return L.hdsm_track_states_host(m, n, ids, planned, T, rnd, flown, dist)

    def model(**kw):
        m = sc.gust_model(**MODEL)
        for k, (ax, v) in kw.items():
            getattr(m, k)[ax] = v
        return m

    bad_models = [model(wind=(0, np.nan)), model(wind=(2, np.inf)), model(gust=(1, np.nan)), model(jitter=(2, -np.inf)), model(gust=(0, -1e-9)),
                  model(jitter=(1, -0.5))]
    for m in bad_models:
        assert rc(m=m) == lib.HDSM_ERR_BAD_ARG
    for kw in (dict(m=None), dict(ids=None), dict(planned=None), dict(flown=None), dict(n=-1), dict(T=0.0), dict(T=-0.1), dict(T=np.nan),
               dict(T=np.inf), dict(rnd=-1), dict(rnd=2 ** 40 + 1)):
        assert rc(**kw) == lib.HDSM_ERR_BAD_ARG, kw
    assert (flown == -7.0).all() and (dist == -7.0).all()                    # a refusal writes nothing
    assert rc(n=0, ids=None, planned=None, flown=None, dist=None) == 0 and rc(rnd=2 ** 40) == 0 and not (flown == -7.0).any()
    with pytest.raises(lib.HdsmError) as e:
        lib.track_states(bad_models[0], ids, planned, 0.1)
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: hdsm_track_states_host"
    with pytest.raises(lib.HdsmError):
        lib.track_states(good, ids, np.ones((2, 9)), 0.1)
    # the mirror and the device loop refuse the same models, and null handles
    prm, cfg = lc.shape_params(lc.SHAPES[0])
    shard = swarm.SwarmShard(prm, cfg, 2, 0, np.zeros((2, 3)), np.ones((2, 3)))
    before = lc.agents_bytes(co.export_agents(shard)[0])
    for m in bad_models:
        with pytest.raises(lib.HdsmError):
            shard.set_tracking(m)
    assert L.hdsm_swarm_set_states(shard.h, None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_swarm_track_records(shard.h, None) == lib.HDSM_ERR_BAD_ARG
    assert lc.agents_bytes(co.export_agents(shard)[0]) == before and not shard.track_records()["rounds"].any()
    for fn, args in (("hdsm_swarm_set_tracking", (good,)), ("hdsm_swarm_set_states", (planned, None)), ("hdsm_swarm_track_records", (np.zeros(1, lib.TRACK_RECORD),)),
                     ("hdsm_dswarm_set_tracking", (good,)), ("hdsm_dswarm_set_states", (planned, None)), ("hdsm_dswarm_set_states_device", (None, None, None)),
                     ("hdsm_dswarm_track_records", (np.zeros(1, lib.TRACK_RECORD),)), ("hdsm_dswarm_track_stats", (np.zeros(3, np.int64),)),
                     ("hdsm_dswarm_plans_device", (C.byref(C.c_void_p()), C.byref(C.c_void_p())))):
        assert getattr(L, fn)(None, *args) == lib.HDSM_ERR_BAD_ARG, fn


def test_the_binding_and_the_helpers():
    f64, u8, i64, i32 = (lib.CTYPES[t] for t in ("double*", "uint8_t*", "int64_t*", "int32_t*"))
    trk, rec = lib.CTYPES["hdsm_tracking*"], lib.CTYPES["hdsm_track_record*"]
    want = {"hdsm_track_states_host": [trk, C.c_int32, i32, f64, C.c_double, C.c_int64, f64, f64],
            "hdsm_track_states_batch": [C.c_int32, trk, C.c_int32, i32, f64, C.c_double, C.c_int64, f64, f64],
            "hdsm_swarm_set_tracking": [C.c_void_p, trk], "hdsm_swarm_set_states": [C.c_void_p, f64, u8], "hdsm_swarm_track_records": [C.c_void_p, rec],
            "hdsm_dswarm_set_tracking": [C.c_void_p, trk], "hdsm_dswarm_set_states": [C.c_void_p, f64, u8],
            "hdsm_dswarm_set_states_device": [C.c_void_p, f64, u8, C.c_void_p], "hdsm_dswarm_track_records": [C.c_void_p, rec],
            "hdsm_dswarm_track_stats": [C.c_void_p, i64], "hdsm_dswarm_plans_device": [C.c_void_p, lib.CTYPES["void**"], lib.CTYPES["void**"]]}
    L = lib.load()
    for name, argtypes in want.items():
        restype, got = lib.SIGNATURES[name]
        assert restype is C.c_int and got == argtypes and hasattr(L, name), name
    assert trk is C.POINTER(Tracking) and rec.dtype == lib.TRACK_RECORD
    assert [(n, lib.TRACK_RECORD.fields[n][1]) for n in lib.TRACK_RECORD.names] == [(n, getattr(TrackRecord, n).offset) for n, _ in TrackRecord._fields_]
    m = sc.gust_model(2 ** 64 - 1, (1, 2, 3), (4, 5, 6), (7, 8, 9))
    assert (m.seed, list(m.wind), list(m.gust), list(m.jitter)) == (2 ** 64 - 1, [1, 2, 3], [4, 5, 6], [7, 8, 9])
    # the three figures of tracking_error.py from the records, against numpy on the samples themselves
    recs, samples = np.zeros(3, lib.TRACK_RECORD), []
    for k, ds in enumerate(([0.1, 0.4], [0.25], [])):
        r = tc.Record()
        for i, d in enumerate(ds):
            r.book(d, 2.0 * d, external=bool(i))
            samples.append(d)
        recs[k] = r.tuple()
    got = swarm.tracking_summary(recs)
    assert got["samples"] == 3 and got["max"] == 0.4 and got["dvel_max"] == 0.8
    assert abs(got["mean"] - np.mean(samples)) < 1e-15 and abs(got["std"] - np.std(samples)) < 1e-12
    assert swarm.tracking_summary(recs[2:]) == dict(samples=0, mean=0.0, std=0.0, max=0.0, dvel_max=0.0)
    # flown_records: (state before, state after) per round
    hist = np.arange(2 * 3 * 9, dtype=np.float64).reshape(2, 3, 9) + 100.0
    starts = np.arange(9.0).reshape(3, 3)
    fr = swarm.flown_records(hist, starts)
    assert fr.shape == (2, 3, 2, 9) and fr.flags.c_contiguous
    assert (fr[0, :, 0, :3] == starts).all() and (fr[0, :, 0, 3:] == 0).all() and (fr[:, :, 1] == hist).all() and (fr[1, :, 0] == hist[0]).all()


def _flight(oracle, model):
    starts, goals = (x[:N_FLIGHT] for x in lc.make_scene(0))
    ctx, loop = lc.make_flight(oracle, lc.SHAPES[0], starts=starts, goals=goals)
    if model is not None:
        loop.shard.set_tracking(model)
    return ctx, loop


def _agents(loop):
    ag = co.export_agents(loop.shard)[0]
    return [dict(state=lc.arr(ag[a].state_curr, 9), traj=lc.arr(ag[a].traj_curr, co.MAXH + 1, 9), has=int(ag[a].has_traj), id=int(ag[a].id))
            for a in range(loop.shard.n_local)]


def test_the_host_mirror_flies_the_model(oracle):
    model = sc.gust_model(**MODEL)
    ctx, loop = _flight(oracle, model)
    step, T = ctx.cfg.step_plan, float(ctx.cfg.step_plan) * ctx.prm.dt
    want = [tc.Record() for _ in range(N_FLIGHT)]
    flown_before, moved = None, 0.0
    for r in range(ROUNDS_FLIGHT):
        rec = []
        loop.step(rec)
        if flown_before is not None:                                         # the solver's x_0 is the state that was flown
            assert rec[0]["state"].tobytes() == flown_before.tobytes(), r
        ag = _agents(loop)
        assert all(a["has"] == 1 and a["id"] == k for k, a in enumerate(ag))
        planned = np.array([a["traj"][step] for a in ag])
        assert (loop.plans_all[:, step] == planned).all() and (loop.has_plan == 1).all()      # the published record stays the plan
        flown, dist = lib.track_states(model, np.arange(N_FLIGHT, dtype=np.int32), planned, T, r)
        state = np.array([a["state"] for a in ag])
        assert state.tobytes() == flown.tobytes(), r
        for k in range(N_FLIGHT):
            f, d, dv = tc.flown(model, k, r, T, planned[k])
            assert f.tobytes() == state[k].tobytes() and d == dist[k]
            want[k].book(d, dv)
        assert tc.records_equal(loop.shard.track_records(), want), r
        moved = max(moved, float(dist.max()))
        flown_before = state
    assert moved > 1e-3
    summary = swarm.tracking_summary(loop.shard.track_records())
    print(summary)
    assert summary["samples"] == N_FLIGHT * ROUNDS_FLIGHT and 0 < summary["mean"] <= summary["max"] == max(w.dist_max for w in want)
    # off: the records are kept, the next commit lands on the plan again; on again: the tracking round restarts at 0
    loop.shard.set_tracking(None)
    loop.step()
    ag = _agents(loop)
    assert all((a["state"] == a["traj"][step]).all() for a in ag) and tc.records_equal(loop.shard.track_records(), want)
    loop.shard.set_tracking(model)
    loop.step()
    ag = _agents(loop)
    for k, a in enumerate(ag):
        assert a["state"].tobytes() == tc.flown(model, k, 0, T, a["traj"][step])[0].tobytes()


def test_states_from_outside_on_the_host_mirror(oracle):
    ctx, loop = _flight(oracle, None)
    for _ in range(2):
        loop.step()
    before = np.array([a["state"] for a in _agents(loop)])
    given = before + np.arange(N_FLIGHT * 9).reshape(N_FLIGHT, 9) * 1e-3 + 0.01
    given[2, 4] = np.nan                                                     # a row that is skipped and counted nowhere
    mask = np.array([1, 0, 1, 1], np.uint8)
    loop.shard.set_states(given, mask)
    after = np.array([a["state"] for a in _agents(loop)])
    assert after[[0, 3]].tobytes() == given[[0, 3]].tobytes() and after[[1, 2]].tobytes() == before[[1, 2]].tobytes()
    want = [tc.Record() for _ in range(N_FLIGHT)]
    for k in (0, 3):
        want[k].book(tc.norm3(*(given[k, :3] - before[k, :3])), tc.norm3(*(given[k, 3:6] - before[k, 3:6])), external=True)
    assert tc.records_equal(loop.shard.track_records(), want)
    rec = []
    loop.step(rec)                                                           # the next round is solved from what was given
    assert rec[0]["state"].tobytes() == after.tobytes()
    loop.shard.set_states(before)                                            # no mask: everybody
    assert np.array([a["state"] for a in _agents(loop)]).tobytes() == before.tobytes()
    assert loop.shard.track_records()["external"].tolist() == [2, 1, 1, 2]


def test_a_mirror_that_never_sets_a_model_is_todays(oracle):
    """Two flights, one of which sets a model and takes it back before its first round: the same bytes in every agent state after
    every round, and state_curr = traj_curr[step_plan], as without this feature."""
    (ctx, plain), (_, unset) = _flight(oracle, None), _flight(oracle, sc.gust_model(**MODEL))
    unset.shard.set_tracking(None)
    for r in range(ROUNDS_FLIGHT):
        plain.step(), unset.step()
        assert lc.agents_bytes(co.export_agents(plain.shard)[0]) == lc.agents_bytes(co.export_agents(unset.shard)[0]), r
        assert plain.plans_all.tobytes() == unset.plans_all.tobytes()
        assert all((a["state"] == a["traj"][ctx.cfg.step_plan]).all() for a in _agents(plain))
    assert not plain.shard.track_records()["rounds"].any() and not unset.shard.track_records()["rounds"].any()
