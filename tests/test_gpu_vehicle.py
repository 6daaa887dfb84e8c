"""A vehicle in the device loop on the MI355X (hdsm_dswarm_set_vehicle / _vehicle_states* / _vehicle_stats, hdsm_vehicle_fly_batch,
k_vehicle; include/hdsm_swarm.h). 8 agents on the 4 m circle of tests/test_vehicle.py:

  * batch equals host: hdsm_vehicle_fly_batch equals hdsm_vehicle_fly_host bit for bit on every case of tests/vehicle_cases.py and at
    n = 1, 63, 64, 65, 130 crossed with step_plan 1, 3 and n_sub 1, 10;
  * the device loop against the host mirror that follows it, after each of 12 rounds, H = 10 and 15, seven flavours: for the same
    setpoints the vehicle states, the poses, state_curr, the counters and the track records agree bit for bit;
  * the flight against a host mirror flown on its own with the same vehicle: statuses equal, plans within 1e-7 — and not vacuous: it
    leaves the vehicle-less flight by what tests/test_vehicle.py recorded on the CPU, with the same count of unsolved instances;
  * off is off; a flight taken over and handed back keeps every vehicle's 128 bytes; local ranks; the device pointer; resources.

Tolerances: those of tests/test_gpu_tracking.py (device loop against host mirror): statuses equal, plans 1e-7."""
import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
import tracking_cases as tc
import vehicle_cases as vc
from flight_harness import MirroredRank, device_loop, hdsm, raw  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import assert_no_scratch_no_lds
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.lib import VEHICLE_STATE
from multi_agent_pkgs_amd.params import agile_params
from vehicle_cases import N_ROB, RECORDED, gusty, scenario

pytestmark = pytest.mark.gpu

PLAN_TOL, ROUNDS = 1e-7, 12
ZERO_VEHICLE = bytes(128)


def test_the_batch_equals_the_host_form_bit_for_bit(hdsm):  # noqa: F811
    n_cases, reseated = 0, 0
    for name, m, ids, q, step, dt, start, sps, planned, vss, _ in vc.cases():
        args = (m, ids, start, vc.command_array(sps), planned, vc.vstate_array(vss), step, dt, q)
        host, dev = hdsm.vehicle_fly(*args), hdsm.vehicle_fly(*args, device=0)
        assert all(h.tobytes() == d.tobytes() for h, d in zip(host[:4], dev[:4])) and host[4] == dev[4], name
        n_cases, reseated = n_cases + 1, reseated + dev[4][1]
    assert n_cases == vc.N_CASES and reseated == vc.N_CASES // 2
    rng = np.random.default_rng(5)
    for size in (1, 63, 64, 65, 130):                                          # both sides of the workgroup boundary, more than two blocks
        for step in (1, 3):
            for n_sub in (1, 10):
                m = gusty(n_sub=n_sub, feed=size % 2, acc_from=step % 2)
                ids = rng.integers(0, 2 ** 31 - 1, size, dtype=np.int32)
                start = rng.uniform(-3.0, 3.0, (size, 9))
                sp = np.zeros((size, step), hdsm.COMMAND)
                sp["pos"], sp["vel"], sp["acc"] = (start[:, None, 3 * c:3 * c + 3] + rng.uniform(-0.3, 0.3, (size, step, 3)) for c in range(3))
                sp["yaw"], sp["valid"], sp["quat"][..., 3] = rng.uniform(-3.0, 3.0, (size, 1)), 1, 1.0
                vs = hdsm.vehicle_seat(m, start, rng.uniform(-3.0, 3.0, size))
                vs["omega"] = rng.uniform(-1.0, 1.0, (size, 3))
                args = (m, ids, start, sp, start + 0.01, vs, step, 0.1, 9)
                host, dev = hdsm.vehicle_fly(*args), hdsm.vehicle_fly(*args, device=0)
                assert all(h.tobytes() == d.tobytes() for h, d in zip(host[:4], dev[:4])) and host[4] == dev[4], (size, step, n_sub)
                assert host[4][0] == size and np.isfinite(host[1]).all()
    L = hdsm.load()
    bad = gusty()
    bad.tau_rate = 0.0
    flown = np.full((2, 9), -7.0)
    vs = hdsm.vehicle_seat(gusty(), np.ones((2, 9)), np.zeros(2))
    sp = np.zeros((2, 1), hdsm.COMMAND)
    for model, q in ((bad, 0), (gusty(), 2 ** 40 + 1)):
        assert L.hdsm_vehicle_fly_batch(0, model, 2, np.arange(2, dtype=np.int32), 1, 0.1, q, np.ones((2, 9)), sp, np.ones((2, 9)), vs, flown, None, None,
                                        None) == hdsm.HDSM_ERR_BAD_ARG
    assert (flown == -7.0).all()


class VRank(MirroredRank):
    """tests/flight_harness.py's MirroredRank — a device shard with the host mirror that follows it: before a round the mirror takes the device's
    flight (agents, yaw, vehicles), after it the device's solutions, and commits them itself — with a vehicle on both."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.veh, self.q, self.rounds_veh = None, 0, 0
        self.stats = np.zeros(4, np.int64)

    def set_vehicle(self, m):
        self.dsw.download(states=True)
        self.dsw.set_vehicle(m), self.mirror.set_vehicle(m)
        self.veh, self.q = m, 0
        fly = self.n_fly
        assert self.dsw.vehicle_states()[:fly].tobytes() == self.mirror.vehicle_states()[:fly].tobytes()

    def before_round(self):
        super().before_round()
        self.vs_before = self.dsw.vehicle_states() if self.veh is not None else None

    def feature_round(self, tag, ref_full, out, after, state):
        n, fly, first, traj = self.n, self.n_fly, self.mirror.first_id, out["traj"]
        sp, pose = self.dsw.commands()
        m_sp, m_pose, m_yaw = self.mirror.commands()
        assert sp[:fly].tobytes() == m_sp[:fly].tobytes() and pose[:fly].tobytes() == m_pose[:fly].tobytes(), tag
        assert self.dsw.track_records()[:fly].tobytes() == self.mirror.track_records()[:fly].tobytes(), tag
        if self.veh is None:
            return
        self.rounds_veh += 1
        vs = self.dsw.vehicle_states()
        assert vs[:fly].tobytes() == self.mirror.vehicle_states()[:fly].tobytes(), tag
        assert all(vs[k].tobytes() == ZERO_VEHICLE for k in range(fly, n)), tag  # the scripted tail is never touched
        assert (pose["quat"][:fly] == vs["quat"][:fly]).all() and (pose["pos"][:fly] == vs["pos"][:fly]).all(), tag
        # ... and the host form on plain arrays, which also says what the counters must show
        step = sp.shape[1]
        has_traj = np.array([after[k].has_traj for k in range(fly)], bool)
        pre_state = np.array([lc.arr(self.pre[k].state_curr, 9) for k in range(fly)])
        planned = np.where(has_traj[:, None], traj[:fly, step], pre_state)
        ids = np.arange(first, first + fly, dtype=np.int32)                     # GLOBAL ids
        h_vs, h_flown, _, h_pose, stats = hdsm_lib().vehicle_fly(self.veh, ids, traj[:fly, 0], sp[:fly], planned, self.vs_before[:fly], step, self.prm.dt,
                                                                 self.q)
        assert h_vs.tobytes() == vs[:fly].tobytes() and h_pose.tobytes() == pose[:fly].tobytes() and h_flown.tobytes() == state[:fly].tobytes(), tag
        self.q += 1
        self.stats += stats
        want = dict(zip(("flown", "reseated", "thrust_clamped", "rate_clamped"), (int(x) for x in self.stats)), launches=self.rounds_veh if fly else 0)
        assert self.dsw.vehicle_stats() == want, tag


def hdsm_lib():
    from multi_agent_pkgs_amd import lib
    return lib


def _one_rank(hdsm, prm, n_script=0):  # noqa: F811
    starts, goals = scenario()
    cfg = swarm.default_swarm_config()
    sol = hdsm.Solver(prm, N_ROB, N_ROB)
    shard = swarm.SwarmShard(prm, cfg, N_ROB, 0, starts, goals)
    dsw = swarm.DeviceSwarm(shard, sol)
    return sol, VRank(dsw, prm, cfg, starts, goals, n_fly=N_ROB - n_script)


FLAVOURS = ["plain", "gusty", "along", "acc-from-model", "scripted-tail", "states-from-outside", "switched-on-at-4"]


@pytest.mark.parametrize("n_hor", [10, 15])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_device_loop_is_its_host_mirror(hdsm, flavour, n_hor):  # noqa: F811
    prm = agile_params(n_hor, max_rows_static=18)
    sol, rank = _one_rank(hdsm, prm, n_script=2 if flavour == "scripted-tail" else 0)
    m = dict(plain=sc.crazyflie_vehicle(), along=gusty(feed=1), **{"acc-from-model": gusty(acc_from=1)}).get(flavour, gusty())
    on_at = 4 if flavour == "switched-on-at-4" else 0
    if flavour == "scripted-tail":
        rank.dsw.set_script(sc.stack_tracks(sc.hold_track((20.0, 15.0, 1.5)), sc.line_track((16.0, 12.0, 1.5), (16.0, 18.0, 1.5), 1.0)), 0)
    rank.set_commands(True, yaw0=np.linspace(-3.0, 3.0, N_ROB))
    for r in range(ROUNDS):
        if r == on_at:
            rank.set_vehicle(m)
        rank.before_round()
        rank.dsw.round()
        rank.after_round((flavour, r))
        if flavour == "states-from-outside" and r == 5:                         # measured states re-seat the vehicles, on both sides
            rank.dsw.download(states=True)
            s = np.array([lc.arr(a.state_curr, 9) for a in co.export_agents(rank.mirror)[0]])
            s[:, :3] += 0.05 * np.array([1.0, -1.0, 0.5])
            mask = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
            before = rank.dsw.vehicle_states()
            rank.dsw.set_states(s, mask), rank.mirror.set_states(s, mask)
            vs = rank.dsw.vehicle_states()
            assert vs.tobytes() == rank.mirror.vehicle_states().tobytes() and vs[mask == 0].tobytes() == before[mask == 0].tobytes()
            assert (vs["pos"][mask == 1] == s[mask == 1, :3]).all() and not vs["omega"][mask == 1].any()
    stats = rank.dsw.vehicle_stats()
    assert stats["launches"] == ROUNDS - on_at and stats["flown"] == (ROUNDS - on_at) * rank.n_fly and stats["reseated"] == 0
    recs = rank.dsw.track_records()
    assert (recs["rounds"][:rank.n_fly] == ROUNDS - on_at).all() and not recs["rounds"][rank.n_fly:].any()
    if flavour != "plain":
        assert recs["dist_max"][:rank.n_fly].min() > 1e-3                       # the gusts were flown
    print(flavour, n_hor, stats, swarm.tracking_summary(recs[:rank.n_fly]))
    rank.dsw.close(), sol.close()


def _fly(hdsm, prm, m, rounds):  # noqa: F811
    """a device flight on its own: per round the plans, flags and statuses"""
    starts, goals = scenario()
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), N_ROB, starts=starts, goals=goals)
    dsw = swarm.DeviceSwarm(loop.shard, sol)
    if m is not None:
        dsw.set_commands(True), dsw.set_vehicle(m)
    out = []
    for r in range(rounds):
        dsw.round()
        plans, has, status, _ = dsw.download(states=False)
        out.append(dict(plans=plans, has=has, status=status))
    got = dict(rounds=out, records=dsw.track_records(), vs=dsw.vehicle_states() if m is not None else None)
    dsw.close(), sol.close()
    return got


@pytest.mark.parametrize("n_hor", [10, 15])
def test_the_flight_is_its_host_mirror(hdsm, n_hor):  # noqa: F811
    """The device flight against a host mirror flown on its own (SwarmLoop on the same device solver) with the same vehicle on both: the
    solver's differences pass through the vehicle's gains into the next round's x_0, so this is where feedback could amplify them."""
    prm, m, rounds = agile_params(n_hor, max_rows_static=18), gusty(), 14
    dev = _fly(hdsm, prm, m, rounds)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), N_ROB, starts=scenario()[0], goals=scenario()[1])
    loop.shard.set_commands(True), loop.shard.set_vehicle(m)
    worst = 0.0
    for r, d in enumerate(dev["rounds"]):
        out = loop.step()
        assert (d["has"] == loop.has_plan).all() and (d["status"] == out["status"]).all(), (r, d["status"].tolist(), out["status"].tolist())
        err = float(np.abs(d["plans"] - loop.plans_all).max())
        worst = max(worst, err)
        print(f"H = {n_hor} round {r}: max |plans - mirror| {err:.3e}")
        assert err < PLAN_TOL, (r, err)
    vs, mv = dev["vs"], loop.shard.vehicle_states()
    print(f"H = {n_hor}: {rounds} rounds, max |plans - mirror| {worst:.3e}, max |vehicle pos - mirror| {np.abs(vs['pos'] - mv['pos']).max():.3e}")
    assert np.abs(vs["pos"] - mv["pos"]).max() < PLAN_TOL
    rec, mrec = dev["records"], loop.shard.track_records()
    assert (rec["rounds"] == mrec["rounds"]).all() and np.abs(rec["dist_sum"] - mrec["dist_sum"]).max() < rounds * PLAN_TOL
    sol.close()


def test_the_vehicle_leaves_the_vehicle_less_flight(hdsm):  # noqa: F811
    """Not vacuous: the figures tests/test_vehicle.py recorded on the CPU with the oracle as the solver (RECORDED) hold for what the device
    flies. The distance is compared to 1e-3 m: the solver agrees with the oracle to 1e-6 and 14 rounds of feedback lie between."""
    prm, rounds = agile_params(10, max_rows_static=18), 14
    with_v, without = _fly(hdsm, prm, gusty(), rounds), _fly(hdsm, prm, None, rounds)
    leaves = max(float(np.abs(a["plans"][:, :, :3] - b["plans"][:, :, :3]).max()) for a, b in zip(with_v["rounds"], without["rounds"]))
    unsolved = sum(int((a["status"] == 2).sum()) for a in with_v["rounds"])
    print(f"leaves the vehicle-less flight by {leaves:.6f} m, {unsolved} of {N_ROB * rounds} instances without a solution;",
          swarm.tracking_summary(with_v["records"]))
    assert leaves > 1e-3 and abs(leaves - RECORDED["leaves_by"]) < 1e-3 and unsolved == RECORDED["unsolved"]
    assert not without["records"]["rounds"].any()


def test_off_is_off_and_the_refusals(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    (sol0, plain), (sol1, unset) = _one_rank(hdsm, prm), _one_rank(hdsm, prm)
    plain, unset = plain.dsw, unset.dsw
    plain.set_history(6), unset.set_history(6)
    zero = dict(launches=0, flown=0, reseated=0, thrust_clamped=0, rate_clamped=0)

    def refused(fn, *a):
        with pytest.raises(hdsm.HdsmError) as e:
            fn(*a)
        return e.value.code == hdsm.HDSM_ERR_BAD_ARG and "hdsm_dswarm_" in str(e.value)

    assert refused(plain.vehicle_states) and refused(plain.vehicle_states_device)   # no buffers before the first setting
    assert refused(unset.set_vehicle, gusty())                                      # commands off
    unset.set_commands(True)
    unset.set_tracking(sc.gust_model(1, gust=(1.0, 1.0, 1.0)))
    assert refused(unset.set_vehicle, gusty())                                      # a tracking model on
    unset.set_tracking(None)
    bad = gusty()
    bad.rate_max[1] = 0.0
    assert refused(unset.set_vehicle, bad) and refused(unset.vehicle_states) and unset.vehicle_stats() == zero
    unset.set_vehicle(gusty())
    assert refused(unset.set_tracking, sc.gust_model(1)) and refused(unset.set_commands, False)
    unset.set_vehicle(None), unset.set_commands(False)
    plain.set_vehicle(None)                                                         # off on a dswarm that never had one: a no-op
    for r in range(6):
        plain.round(), unset.round()
        assert raw(plain).tobytes() == raw(unset).tobytes(), r
    assert plain.history(mirror=False)[0].tobytes() == unset.history(mirror=False)[0].tobytes()
    assert plain.vehicle_stats() == zero and unset.vehicle_stats() == zero and refused(plain.vehicle_states_device)
    assert not unset.track_records()["rounds"].any()
    for x in (plain, unset, sol0, sol1):
        x.close()


def test_a_flight_taken_over_and_handed_back_keeps_every_vehicle(hdsm):  # noqa: F811
    prm, m = agile_params(10, max_rows_static=18), gusty(feed=1)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), N_ROB, starts=scenario()[0], goals=scenario()[1])
    loop.shard.set_commands(True), loop.shard.set_vehicle(m)
    for _ in range(3):
        loop.step()
    mine = loop.shard.vehicle_states()
    assert np.abs(mine["omega"]).max() > 1e-3                                   # vehicles in motion, not freshly seated ones
    dsw = swarm.DeviceSwarm(loop.shard, sol)                                    # nothing is set on the dswarm: it takes setting and vehicles
    assert dsw.vehicle_states().tobytes() == mine.tobytes()
    dsw.upload_plans(loop.plans_all, loop.has_plan)
    dsw.round(), dsw.round()
    there = dsw.vehicle_states()
    assert dsw.vehicle_stats()["launches"] == 2 and there.tobytes() != mine.tobytes()
    dsw.download(states=True)
    assert loop.shard.vehicle_states().tobytes() == there.tobytes()
    # ... and the vehicle round travelled too: the mirror's next round is the device's next round
    plans_before = dsw.download(states=False)[:2]
    loop.plans_all, loop.has_plan = plans_before[0][:N_ROB].copy(), plans_before[1][:N_ROB].copy()
    out = loop.step()
    dsw.round()
    plans, has, status, _ = dsw.download(states=False)
    assert (status == out["status"]).all() and np.abs(plans - loop.plans_all).max() < PLAN_TOL
    assert np.abs(dsw.vehicle_states()["pos"] - loop.shard.vehicle_states()["pos"]).max() < PLAN_TOL
    dsw.close(), sol.close()


@pytest.mark.parametrize("n_rob,world", [(10, 3), (5, 4)])
def test_local_ranks_fly_their_own_vehicles(hdsm, n_rob, world):  # noqa: F811
    """Every rank is its own mirror bit for bit, the host form called with GLOBAL ids — the draws a one-rank flight makes."""
    prm, cfg = agile_params(10, max_rows_static=18), swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(n_rob, radius=4.0)
    flock = swarm.LocalRanks(prm, cfg, n_rob, world, starts=starts, goals=goals)
    ranks = []
    for r, d in enumerate(flock.dswarms):
        first, n_local = swarm.shard_range(n_rob, r, world)
        ranks.append(VRank(d, prm, cfg, starts[first:first + n_local], goals[first:first + n_local]))
        ranks[-1].set_commands(True)
        ranks[-1].set_vehicle(gusty())
    assert [k.n for k in ranks] == ([4, 4, 2] if world == 3 else [2, 2, 1, 0])
    for r in range(6):
        for k in ranks:
            k.before_round()
        flock.round(None)
        for i, k in enumerate(ranks):
            k.after_round((r, i))
    for k in ranks:
        assert k.dsw.vehicle_stats()["launches"] == (6 if k.n else 0)
    # the one-rank flight of the same swarm
    sol = hdsm.Solver(prm, n_rob, n_rob)
    one = swarm.DeviceSwarm(swarm.SwarmShard(prm, cfg, n_rob, 0, starts, goals), sol)
    one.set_commands(True), one.set_vehicle(gusty())
    for r in range(6):
        one.round()
    pos = np.concatenate([k.dsw.vehicle_states()["pos"] for k in ranks if k.n])
    assert np.abs(pos - one.vehicle_states()["pos"]).max() < PLAN_TOL
    one.close(), sol.close(), flock.close()


class _DeviceBytes:
    """A device address as something torch.as_tensor takes"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(int(nbytes),), typestr="|u1", data=(int(ptr), False), version=2)


def test_the_device_pointer(hdsm):  # noqa: F811
    import torch
    prm = agile_params(10, max_rows_static=18)
    sol, rank = _one_rank(hdsm, prm)
    rank.dsw.set_commands(True), rank.dsw.set_vehicle(gusty())
    d_vs = rank.dsw.vehicle_states_device()
    stream = torch.cuda.current_stream()
    for r in range(3):
        rank.dsw.round(stream=stream)
        stream.synchronize()
        seen = torch.as_tensor(_DeviceBytes(d_vs, N_ROB * 128), device="cuda").cpu().numpy().view(VEHICLE_STATE)
        assert seen.tobytes() == rank.dsw.vehicle_states().tobytes() and np.isfinite(seen["pos"]).all(), r
        assert rank.dsw.vehicle_states_device() == d_vs
    rank.dsw.close(), sol.close()


def test_k_vehicle_uses_no_scratch_and_no_lds(tmp_path):
    # (scalar registers parked in the lanes of a vector register are neither: k_vehicle holds a 224-byte setting and parks some of
    # the pointers of its prologue and epilogue there, none inside the sub-step loop — DESIGN §8)
    assert_no_scratch_no_lds(tmp_path, "k_vehicle", scalar_spills=True)
    assert_no_scratch_no_lds(tmp_path, "k_seat", scalar_spills=True)
