"""The flight audit on the MI355X (csrc/audit_kernels.hip): the device batch against the host form bit for bit, the audit of the
device-resident loop against the host form and the numpy restatement on the records of every round, the state history, a flight
taken over in mid-air, and the off switch."""
import ctypes as C

import numpy as np
import pytest

import audit_cases as ac
import dmp_cases as dc
from audit_cases import CLEAR, check_separation, check_track
from flight_harness import device_loop, hdsm  # noqa: F401  (hdsm: the module's fixture)
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import agile_params

pytestmark = pytest.mark.gpu


def _same(dev, host):
    for f in host.dtype.names:
        assert np.array_equal(dev[f], host[f]), (f, np.nonzero(dev[f] != host[f])[0][:8], dev[f][dev[f] != host[f]][:4], host[f][dev[f] != host[f]][:4])
    assert dev.tobytes() == host.tobytes()


def test_flight_audit_batch_equals_the_host_form(hdsm):  # noqa: F811
    """hdsm_flight_audit_batch == hdsm_flight_audit_host on every field, bit for bit: the 320 random batches of the CPU test, subject
    windows, 2 240 tracks in cfg 3's inflated and pre-processed forest, 4096 agents of cfg 5's lattice in its pre-processed world with
    n_hor = 15 (step_plan 1 and 3: 64 x 64 workgroups), and a 1024-agent ring at the separation limit. The
    large batches are also compared with the numpy restatement."""
    rng = np.random.default_rng(2024)
    rows = 0
    for t in range(320):
        plans, has, S, (r, z) = ac.random_batch(rng, step_plan=1 + t % 2, aniso=bool((t // 2) % 2))
        host = hdsm.flight_audit_host(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z)
        _same(hdsm.flight_audit_batch(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z), host)
        rows += plans.shape[0]
        if t % 40 == 0 and plans.shape[0] > 4:
            first, n_local = plans.shape[0] // 3, plans.shape[0] // 2
            _same(hdsm.flight_audit_batch(plans, has, step_plan=S, first=first, n_local=n_local, drone_radius=r, drone_z_offset=z),
                  host[first:first + n_local])
    assert rows > 10000
    # step_plan up to the horizon: fewer partners fit a tile (4 sub-steps: 51 partners, 14 chunks)
    plans, has, _, (r, z) = ac.random_batch(rng, n=700, step_plan=1)
    for S in (3, ac.N_HOR):
        _same(hdsm.flight_audit_batch(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z),
              hdsm.flight_audit_host(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z))
    # own tracks
    raw, origin = sc.forest_for_circle(48, seed=21)
    tracks = 0
    for world in (sc.inflate(raw), dc.preprocessed(raw, hdsm.map_preprocess)):
        world = world.copy()
        world[:3][world[:3] == 0] = -1
        plans, has, S = ac.tracks_in_world(rng, world, origin, 1120)
        host = hdsm.flight_audit_host(plans, has, step_plan=S, world=world, worigin=origin, voxel_size=0.3)
        _same(hdsm.flight_audit_batch(plans, has, step_plan=S, world=world, worigin=origin, voxel_size=0.3), host)
        assert host["crossed"].sum() > 100 and host["occupied"].sum() > 100 and host["unknown"].sum() > 0
        tracks += 1120
    assert tracks >= 2000
    # cfg 5: the 64 x 64 lattice (2.01 m pitch) a few rounds into its flight, in the forest-wall-forest world with its potential field
    n_y = 64
    starts, _ = sc.lattice_scenario(n_y, n_y)
    rawf, org5 = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
    world5 = dc.preprocessed(rawf, hdsm.map_preprocess)
    n = n_y * n_y
    steps = np.tile([0.6, 0.0, 0.0], (n, 15, 1)) + rng.uniform(-0.25, 0.25, (n, 15, 3))
    plans = ac.records(starts + [4.0, 0.0, 0.0] + rng.uniform(-0.6, 0.6, (n, 3)), steps, vel=rng.uniform(-9, 9, (n, 16, 3)), n_hor=15)
    has = (rng.uniform(size=n) < 0.97).astype(np.uint8)
    for S in (1, 3):
        host = hdsm.flight_audit_host(plans, has, step_plan=S, world=world5, worigin=org5, voxel_size=0.3)
        _same(hdsm.flight_audit_batch(plans, has, step_plan=S, world=world5, worigin=org5, voxel_size=0.3), host)
        assert check_separation(host, plans, has, S, 0, n, 0.25, 0.25) <= 0.02 * n
        assert (np.sqrt(host["sep2"][host["partner"] >= 0]) < 2.5).sum() > 100 and host["pot"].sum() > 0
    check_track(host, plans, has, 3, 0, n, world5, org5)
    _same(hdsm.flight_audit_batch(plans, has, step_plan=1, first=1024, n_local=1024, world=world5, worigin=org5, voxel_size=0.3),
          hdsm.flight_audit_host(plans, has, step_plan=1, world=world5, worigin=org5, voxel_size=0.3)[1024:2048])
    # the ring at the separation limit: every agent has two neighbours at sigma = 1 and many more nearby
    plans, has = ac.ring(1024)
    host = hdsm.flight_audit_host(plans, has, step_plan=2)
    _same(hdsm.flight_audit_batch(plans, has, step_plan=2), host)
    assert (np.sqrt(host["sep2"]) < 1.0).all() and (np.sqrt(host["sep2"]) > 0.97).all()
    nb = (host["partner"] - np.arange(1024)) % 1024
    assert np.isin(nb, (1, 1023)).all()


def _forest_loop(hdsm, n_rob):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    raw, origin = sc.forest_for_circle(n_rob, seed=21)
    world = dc.preprocessed(raw, hdsm.map_preprocess)
    from multi_agent_pkgs_amd import swarm
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
    assert loop.set_world(world, origin) == 0
    return prm, sol, loop, world, origin


def _state_curr(loop, dsw, plans, has):
    """state_curr [n][9] of every agent as the device loop holds it now: the states are downloaded into the host mirror, which hands
    them out with the inputs of a round (hdsm_swarm_prepare; what it changes in the mirror is overwritten by the next download)."""
    dsw.download(states=True)
    return loop.shard.prepare(plans, has)["state"].copy()


def _settle_partners(rep, mine, flown, clear, S, r, z):
    """The report with sep_partner set to numpy's on the rows where the library took numpy's runner-up — allowed only where, in the
    round of the minimum, the runner-up was within CLEAR of it, and only if the library's partner IS that close in that round."""
    assert all(has.all() for _, has in flown)               # sep_round counts an agent's audited rounds: every round, then
    rep2 = rep.copy()
    for k in range(rep.shape[0]):
        rd = int(mine.sep_round[k])
        if rd >= 0 and not clear[rd][k] and rep["sep_partner"][k] != mine.sep_partner[k]:
            assert rep["sep_partner"][k] >= 0
            q, _ = ac.pair_q(flown[rd][0][:, :S + 1, :3], np.array([k]), S, r, z)
            assert abs(q[0, :, rep["sep_partner"][k]].min() - mine.sep2_min[k]) <= CLEAR * mine.sep2_min[k], (k, rd)
            rep2["sep_partner"][k] = mine.sep_partner[k]
    return rep2


def _fly_and_compare(hdsm, prm, loop, dsw, n, rounds, world, origin, mine, exact):  # noqa: F811
    """`rounds` rounds of the device loop; after each the plans are downloaded and the audit of exactly those arrays is formed by the
    host form (bit for bit what the device reports) and by numpy (1e-12, integers exactly; `mine` accumulates numpy's own figures,
    partner included). Returns the plans and flags of the rounds, where numpy's runner-up was clear of the minimum, and state_curr
    after every round."""
    r, z, S = prm.drone_radius, prm.drone_z_offset, 1
    flown, clear, states = [], [], []
    for rd in range(rounds):
        dsw.round()
        plans, has, status, failed = dsw.download(states=False)
        last = dsw.last_audit_round()
        host = hdsm.flight_audit_host(plans, has, step_plan=S, drone_radius=r, drone_z_offset=z, world=world,
                                      worigin=origin if world is not None else (0, 0, 0), voxel_size=0.3)
        _same(last, host)
        check_separation(last, plans, has, S, 0, n, r, z)
        want = check_track(last, plans, has, S, 0, n, world, origin) if world is not None else ac.np_track(plans, has, S, 0, n, None, None, 0.3, None)
        sep2, partner, substep, second, _ = ac.np_separation(plans, has, S, 0, n, r, z)
        mine.add(has, sep2, partner, substep, want)
        exact.add(has, host["sep2"], host["partner"], host["substep"], {f: host[f] for f in ("occupied", "unknown", "crossed", "pot", "dist", "speed")})
        flown.append((plans, has)), clear.append(second - sep2 > CLEAR * sep2)
        states.append(_state_curr(loop, dsw, plans, has))
    return flown, clear, states


def test_device_loop_audit_equals_the_restatement_round_by_round(hdsm, tmp_path):  # noqa: F811
    """48 agents through the pre-processed forest for 30 rounds (the audit switched on in the host mirror before the device loop is
    made) and the 64-agent circle for 40 rounds (switched on with hdsm_dswarm_set_audit): hdsm_dswarm_last_audit_round equals the
    host form on the downloaded records every round, hdsm_dswarm_flight_report the accumulated restatement at the end — integers
    exactly, doubles bit for bit against the host form's accumulation and to 1e-12 against numpy's. The history (capacity = rounds)
    holds state_curr of every round, reaches the mirror once, and hdsm_swarm_shutdown writes it as state_hist_<id>.csv."""
    from multi_agent_pkgs_amd import swarm
    for scene, n, rounds in (("forest", 48, 30), ("circle", 64, 40)):
        if scene == "forest":
            prm, sol, loop, world, origin = _forest_loop(hdsm, n)
            loop.shard.set_audit(True)
            dsw = swarm.DeviceSwarm(loop.shard, sol)
        else:
            prm = agile_params(10, max_rows_static=18)
            sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n)
            world, origin = None, None
            dsw = swarm.DeviceSwarm(loop.shard, sol)
            with pytest.raises(hdsm.HdsmError):
                dsw.flight_report()
            dsw.set_audit(True)
        dsw.set_history(rounds)
        mine, exact = ac.Flight(n, 1), ac.Flight(n, 1)
        flown, clear, states = _fly_and_compare(hdsm, prm, loop, dsw, n, rounds, world, origin, mine, exact)
        rep = dsw.flight_report()
        assert exact.same_as(rep, rtol=0.0) is None, exact.same_as(rep, rtol=0.0)
        assert np.array_equal(rep["sep_round"], mine.sep_round)
        rep2 = _settle_partners(rep, mine, flown, clear, 1, prm.drone_radius, prm.drone_z_offset)
        assert mine.same_as(rep2) is None, mine.same_as(rep2)
        assert (rep["rounds"] == rounds).all()
        summ = swarm.flight_summary(rep)
        print(scene, summ)
        if scene == "forest":
            assert summ["pot_sum"] > 0 and summ["mean_potential"] == summ["pot_sum"] / (n * rounds)
        # the history: state_curr as downloaded after every round, bit for bit; nothing dropped
        hist, dropped = dsw.history()
        assert hist.shape == (rounds, n, 9) and dropped == 0
        for rd in range(rounds):
            assert np.array_equal(hist[rd], states[rd]), rd
        dsw.download(states=True)
        assert np.array_equal(loop.shard.state()[0], hist[-1][:, :3])
        assert loop.shard.flight_report().tobytes() == rep.tobytes()              # the record came back with the states
        hist2, _ = dsw.history()                                                   # a second download delivers nothing again
        assert np.array_equal(hist2, hist)
        buf = C.create_string_buffer(8192)
        assert hdsm.load().hdsm_swarm_shutdown(loop.shard.h, 3, str(tmp_path).encode(), 1, buf, 8192) > 0
        lines = (tmp_path / "state_hist_3.csv").read_text().strip().split("\n")
        assert len(lines) == rounds
        for rd, ln in enumerate(lines):
            want = "%f," % ((rd + 1) * prm.dt * 1) + ",".join("%f" % x for x in hist[rd, 3])
            assert ln == want, (rd, ln, want)
        assert "velocity for agent: 3" in buf.value.decode()
        (tmp_path / "state_hist_3.csv").unlink()
        dsw.close()


def test_history_stops_when_full_and_counts_the_rounds_lost(hdsm):  # noqa: F811
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), 16)
    dsw = swarm.DeviceSwarm(loop.shard, sol)
    with pytest.raises(hdsm.HdsmError):
        dsw.history()                                                              # the history is off
    dsw.set_history(10)
    states = []
    for rd in range(15):
        dsw.round()
        plans, has, _, _ = dsw.download(states=False)
        states.append(_state_curr(loop, dsw, plans, has))
    hist, dropped = dsw.history(mirror=False)
    assert hist.shape == (10, 16, 9) and dropped == 5
    assert np.array_equal(hist, np.array(states[:10]))
    dsw.set_history(0)
    with pytest.raises(hdsm.HdsmError):
        dsw.history()
    dsw.close()


def test_flight_taken_over_in_mid_air_keeps_its_record_and_the_off_switch(hdsm):  # noqa: F811
    """10 host rounds with the audit on, then the device loop for 10 rounds, then the download: the record covers 20 rounds, the
    round of the minimum counts from the first host round. With the audit and the history off nothing is reported or timed."""
    from multi_agent_pkgs_amd import swarm
    n = 32
    prm = agile_params(10, max_rows_static=18)
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n)
    loop.shard.set_audit(True)
    r, z = prm.drone_radius, prm.drone_z_offset
    mine = ac.Flight(n, 1)

    def book(plans, has):
        sep2, partner, substep, second, _ = ac.np_separation(plans, has, 1, 0, n, r, z)
        mine.add(has, sep2, partner, substep, ac.np_track(plans, has, 1, 0, n, None, None, 0.3, None))
        return second - sep2 > 1e-9 * sep2

    clear, flown = [], []
    for _ in range(10):
        loop.step()
        clear.append(book(loop.plans_all, loop.has_plan)), flown.append((loop.plans_all.copy(), loop.has_plan.copy()))
    dsw = swarm.DeviceSwarm(loop.shard, sol)
    dsw.upload_plans(loop.plans_all, loop.has_plan)
    for _ in range(10):
        dsw.round()
        plans, has, _, _ = dsw.download(states=False)
        clear.append(book(plans, has)), flown.append((plans, has))
    dsw.download(states=True)
    rep = loop.shard.flight_report()
    assert rep.tobytes() == dsw.flight_report().tobytes()
    assert (rep["rounds"] == 20).all() and np.array_equal(rep["sep_round"], mine.sep_round)
    rep2 = _settle_partners(rep, mine, flown, clear, 1, r, z)                       # (the circle's two neighbours: see test_flight_audit.py)
    assert mine.same_as(rep2) is None, mine.same_as(rep2)
    dsw.close()
    # the off switch
    sol2, loop2 = device_loop(hdsm, prm, swarm.default_swarm_config(), n)
    dsw = swarm.DeviceSwarm(loop2.shard, sol2)
    dsw.set_phase_timing(True)
    for _ in range(3):
        dsw.round()
    assert dsw.last_audit_ms() == 0.0 and dsw.phase_ms()["k_commit"] > 0
    with pytest.raises(hdsm.HdsmError):
        dsw.flight_report()
    with pytest.raises(hdsm.HdsmError):
        dsw.last_audit_round()
    dsw.set_audit(True)
    dsw.round()
    assert dsw.last_audit_ms() > 0 and (dsw.flight_report()["rounds"] == 1).all()
    dsw.set_audit(False)
    dsw.round()
    assert dsw.last_audit_ms() == 0.0 and (dsw.flight_report()["rounds"] == 1).all()
    # back to the host: a setting made on the device loop comes down with the states, and the host loop audits on
    dsw.set_audit(True)
    dsw.round()
    assert not loop2.shard.audit_on
    loop2.plans_all, loop2.has_plan, _, _ = dsw.download(states=True)
    dsw.close()
    assert loop2.shard.audit_on
    loop2.step()
    assert (loop2.shard.flight_report()["rounds"] == 3).all()
