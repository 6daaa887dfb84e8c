"""Commands for the vehicle in the device loop on the MI355X (hdsm_command_batch, hdsm_dswarm_set_commands / _commands /
_commands_device / _command_stats, k_command; include/hdsm_swarm.h). 8 agents on the turned circle of tests/command_cases.py (radius 4 m)
in free space, 12 rounds:

  * batch equals host: hdsm_command_batch equals hdsm_command_host bit for bit at n = 1, 63, 64, 65, 130 and step_plan 1 and 3, the crafted
    agents of command_cases.py in front;
  * the device loop is its host mirror, bit for bit after every round — setpoints, poses, yaw, counters: plain, with a tracking model, with
    a scripted tail, with states from outside between two rounds, switched on in mid-flight, and as local ranks at (10, 3) and (5, 4);
  * commands do not steer; a flight that never asks for them launches nothing; the device pointers; k_command's resources.

How the mirror follows bit for bit: before a round the device's agent states go into the host mirror (hdsm_dswarm_download); behind it the
round's reference, solver output and status — read back from the device's committed agents through a second shard — are handed to
hdsm_swarm_set_reference / hdsm_swarm_commit of the mirror, which then looks from the same state_curr at the same reference point, commits
the same record and flies the same tracking model. The plans it publishes must be the device's, byte for byte, before anything is compared."""
import numpy as np
import pytest

import command_cases as cc
import corridor_oracle as co
import loop_cases as lc
from flight_harness import MirroredRank, hdsm, model, raw  # noqa: F401  (hdsm: the module's fixture)
from kernel_elf import assert_no_scratch_no_lds
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.lib import COMMAND, command
from multi_agent_pkgs_amd.params import K_P_YAW, YAW_IDX, agile_params

pytestmark = pytest.mark.gpu

N_ROB, ROUNDS = cc.N_FLIGHT, 12
ZERO = np.zeros(1, COMMAND)[0].tobytes()


@pytest.mark.parametrize("step_plan", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_the_batch_equals_the_host_form_bit_for_bit(hdsm, n, step_plan):  # noqa: F811
    case = cc.batch(n, seed=n + step_plan)
    host = hdsm.command(**case, step_plan=step_plan)
    dev = hdsm.command(**case, step_plan=step_plan, device=0)
    assert host[0].tobytes() == dev[0].tobytes(), np.nonzero(host[0] != dev[0])[0]
    for j in range(step_plan):
        bad = [k for k in range(n) if host[1][k, j].tobytes() != dev[1][k, j].tobytes()]
        assert not bad, (j, bad[:4], host[1][bad[0], j], dev[1][bad[0], j])
    bad = [k for k in range(n) if host[2][k].tobytes() != dev[2][k].tobytes()]
    assert not bad, (bad[:4], host[2][bad[0]], dev[2][bad[0]])
    assert host[3] == dev[3] and sum(host[3]) == n
    assert (host[2]["valid"] == 0).sum() > 0 or n == 1
    if n == 130 and step_plan == 1:                                          # a refusal enters no device and writes nothing
        L = hdsm.load()
        pose = np.zeros(n, COMMAND)
        bad_valid = case["valid"].copy()
        bad_valid[129] = 3
        for kw in (dict(valid=bad_valid), dict(yaw=np.full(n, np.nan))):
            a = dict(case, **kw)
            assert L.hdsm_command_batch(0, n, 10, 1, 0.1, 3, 1.0, a["n_ref"], a["ref_point"], a["state_before"], a["records"], a["valid"], a["state_after"],
                                        a["yaw"], None, pose, None) == hdsm.HDSM_ERR_BAD_ARG
        assert not pose["valid"].any()


class Rank(MirroredRank):
    """tests/flight_harness.py's MirroredRank with what the commands add: setpoints, poses, yaw, the host form, the counters."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rounds_on = self.steps = self.skipped = 0

    def empty_round(self, tag):
        if self.on:
            assert self.dsw.commands()[1].size == 0

    def feature_round(self, tag, ref_full, out, after, state):
        n, N, fly, status = self.n, self.prm.n_hor, self.n_fly, out["status"]
        if not self.on:
            return
        self.rounds_on += 1
        sp, pose = self.dsw.commands()
        m_sp, m_pose, m_yaw = self.mirror.commands()
        for k in range(fly):
            assert sp[k].tobytes() == m_sp[k].tobytes(), (tag, k, sp[k], m_sp[k])
            assert pose[k].tobytes() == m_pose[k].tobytes(), (tag, k, pose[k], m_pose[k])
            assert pose[k]["valid"] == 0 or pose[k]["yaw"] == m_yaw[k], (tag, k)
        for k in range(fly, n):                                                # the scripted tail: zeros
            assert pose[k].tobytes() == ZERO and all(sp[k, j].tobytes() == ZERO for j in range(sp.shape[1])), (tag, k)
        # ... and the host form on plain arrays, which also says what the counters must show
        step = sp.shape[1]
        valid = np.array([0 if not after[k].has_traj else (2 if status[k] == 2 else 1) for k in range(fly)], np.int32)
        h_yaw, h_sp, h_pose, stats = command(
            self.yaw[:fly], np.full(fly, N + 1, np.int32), ref_full[:fly, YAW_IDX, :3], np.array([lc.arr(self.pre[k].state_curr, 9) for k in range(fly)]),
            out["traj"][:fly] if fly else np.zeros((0, N + 1, 9)), valid, state[:fly], step_plan=step, dt=self.prm.dt, yaw_idx=YAW_IDX, k_p_yaw=K_P_YAW)
        assert h_sp.tobytes() == sp[:fly].tobytes() and h_pose.tobytes() == pose[:fly].tobytes() and h_yaw.tobytes() == m_yaw[:fly].tobytes(), tag
        self.steps, self.skipped = self.steps + stats[0], self.skipped + stats[1]
        assert self.dsw.command_stats() == dict(launches=self.rounds_on, steps=self.steps, skipped=self.skipped), tag


def _one_rank(hdsm, prm, n_script=0):  # noqa: F811
    starts, goals = cc.exchange()
    cfg = swarm.default_swarm_config()
    sol = hdsm.Solver(prm, N_ROB, N_ROB)
    shard = swarm.SwarmShard(prm, cfg, N_ROB, 0, starts, goals)
    dsw = swarm.DeviceSwarm(shard, sol)
    return sol, Rank(dsw, prm, cfg, starts, goals, n_fly=N_ROB - n_script)


def _fly(rank, rounds=ROUNDS, on_at=0, between=None, yaw0=None):
    for r in range(rounds):
        if r == on_at:
            rank.set_commands(True, yaw0=yaw0)
        rank.before_round()
        rank.dsw.round()
        rank.after_round(r)
        if between is not None:
            between(rank, r)
    return rank.dsw.commands()


@pytest.mark.parametrize("flavour", ["plain", "tracked", "scripted-tail", "states-from-outside", "switched-on-at-4"])
def test_the_device_loop_is_its_host_mirror(hdsm, flavour):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    sol, rank = _one_rank(hdsm, prm, n_script=2 if flavour == "scripted-tail" else 0)
    yaw0 = np.linspace(-3.0, 3.0, N_ROB)                                      # (some agents start looking away: the wrap is flown)
    between = None
    if flavour == "tracked":
        rank.dsw.set_tracking(model()), rank.mirror.set_tracking(model())
    if flavour == "scripted-tail":
        rank.dsw.set_script(sc.stack_tracks(sc.hold_track((20.0, 15.0, 1.5)), sc.line_track((16.0, 12.0, 1.5), (16.0, 18.0, 1.5), 1.0)), 0)
    if flavour == "states-from-outside":
        def between(rank, r):
            if r == 5:
                rank.dsw.download(states=True)
                s = np.array([lc.arr(a.state_curr, 9) for a in co.export_agents(rank.mirror)[0]])
                s[:, :3] += 0.05 * np.array([1.0, -1.0, 0.5])
                rank.dsw.set_states(s)
    sp, pose = _fly(rank, on_at=4 if flavour == "switched-on-at-4" else 0, between=between, yaw0=yaw0)
    stats = rank.dsw.command_stats()
    rounds_on = ROUNDS - (4 if flavour == "switched-on-at-4" else 0)
    assert stats["launches"] == rounds_on and stats["steps"] + stats["skipped"] == rounds_on * rank.n_fly and stats["steps"] > stats["skipped"]
    assert (pose["valid"][:rank.n_fly] >= 1).all() and np.abs(pose["yaw"][:rank.n_fly] - yaw0[:rank.n_fly]).max() > 0.2
    if flavour == "tracked":                                                   # the pose is the FLOWN state, not the planned one
        plans = rank.dsw.download(states=False)[0]
        flown = np.concatenate([pose["pos"], pose["vel"], pose["acc"]], axis=1)
        assert np.abs(flown - plans[:, 1]).max() > 1e-4 and rank.dsw.track_stats()["model_launches"] == ROUNDS
        assert np.concatenate([sp[:, 0]["pos"], sp[:, 0]["vel"], sp[:, 0]["acc"]], axis=1).tobytes() == np.ascontiguousarray(plans[:, 1]).tobytes()
    # the way back: a download into the mirror carries the command yaw
    rank.dsw.download(states=True)
    assert rank.mirror.commands()[2][:rank.n_fly].tobytes() == pose["yaw"][:rank.n_fly].tobytes()
    rank.dsw.close(), sol.close()


def test_a_flight_taken_over_keeps_setting_and_yaw(hdsm):  # noqa: F811
    """hdsm_dswarm_create takes the mirror's command setting and yaw: nothing is set on the dswarm, and it flies its mirror."""
    prm, cfg = agile_params(10, max_rows_static=18), swarm.default_swarm_config()
    starts, goals = cc.exchange()
    yaw0 = np.linspace(2.5, -2.5, N_ROB)
    shard = swarm.SwarmShard(prm, cfg, N_ROB, 0, starts, goals)
    shard.set_commands(True, yaw_idx=2, k_p_yaw=1.5, yaw0=yaw0)
    sol = hdsm.Solver(prm, N_ROB, N_ROB)
    dsw = swarm.DeviceSwarm(shard, sol)
    dsw.round()
    sp, pose = dsw.commands()
    # one round on plain arrays: from yaw0, towards reference point 2, with gain 1.5
    dsw.download(states=True)
    ag = co.export_agents(shard)[0]
    ref = np.array([lc.arr(ag[k].traj_ref, co.MAXH + 1, 6)[2, :3] for k in range(N_ROB)])
    rec = np.array([lc.arr(ag[k].traj_curr, co.MAXH + 1, 9)[:prm.n_hor + 1] for k in range(N_ROB)])
    before = np.zeros((N_ROB, 9))
    before[:, :3] = starts
    want = command(yaw0, np.full(N_ROB, prm.n_hor + 1, np.int32), ref, before, rec, np.ones(N_ROB, np.int32), rec[:, 1], yaw_idx=2, k_p_yaw=1.5)
    assert (pose["valid"] == 1).all() and want[2].tobytes() == pose.tobytes() and want[1].tobytes() == sp.tobytes()
    assert shard.commands()[2].tobytes() == want[0].tobytes() == pose["yaw"].tobytes() and np.abs(want[0] - yaw0).max() > 0.1
    assert dsw.command_stats() == dict(launches=1, steps=N_ROB, skipped=0)
    dsw.close(), sol.close()


@pytest.mark.parametrize("n_rob,world", [(10, 3), (5, 4)])
def test_local_ranks_write_their_own_commands(hdsm, n_rob, world):  # noqa: F811
    prm, cfg = agile_params(10, max_rows_static=18), swarm.default_swarm_config()
    starts, goals = cc.exchange(n=n_rob)
    flock = swarm.LocalRanks(prm, cfg, n_rob, world, starts=starts, goals=goals)
    ranks = []
    for r, d in enumerate(flock.dswarms):
        first, n_local = swarm.shard_range(n_rob, r, world)
        ranks.append(Rank(d, prm, cfg, starts[first:first + n_local], goals[first:first + n_local]))
        ranks[-1].set_commands(True, yaw0=np.linspace(-2.0, 2.0, n_rob)[first:first + n_local])
    assert [k.n for k in ranks] == ([4, 4, 2] if world == 3 else [2, 2, 1, 0])
    for r in range(6):
        for k in ranks:
            k.before_round()
        flock.round(None)
        for i, k in enumerate(ranks):
            k.after_round((r, i))
    for k in ranks:
        assert k.dsw.command_stats()["launches"] == (6 if k.n else 0)
    flock.close()


def test_commands_do_not_steer(hdsm):  # noqa: F811
    prm = agile_params(10, max_rows_static=18)
    (sol0, off), (sol1, on) = _one_rank(hdsm, prm), _one_rank(hdsm, prm)
    off.dsw.set_history(ROUNDS), on.dsw.set_history(ROUNDS)
    on.dsw.set_commands(True, yaw0=np.linspace(-3.0, 3.0, N_ROB))
    for r in range(ROUNDS):
        off.dsw.round(), on.dsw.round()
        assert raw(off.dsw).tobytes() == raw(on.dsw).tobytes(), r
    assert off.dsw.history(mirror=False)[0].tobytes() == on.dsw.history(mirror=False)[0].tobytes()
    assert off.dsw.command_stats() == dict(launches=0, steps=0, skipped=0) and on.dsw.command_stats()["launches"] == ROUNDS
    with pytest.raises(hdsm.HdsmError) as e:
        off.dsw.commands()
    assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "hdsm_dswarm_commands" in str(e.value)
    with pytest.raises(hdsm.HdsmError):
        off.dsw.commands_device()
    for kw in (dict(yaw_idx=11), dict(yaw_idx=-1), dict(k_p_yaw=np.inf), dict(yaw0=np.full(N_ROB, np.nan))):
        with pytest.raises(hdsm.HdsmError) as e:
            off.dsw.set_commands(True, **kw)
        assert e.value.code == hdsm.HDSM_ERR_BAD_ARG and "hdsm_dswarm_set_commands" in str(e.value)
    off.dsw.set_commands(False)                                                # off on a dswarm that never had them: a no-op
    assert off.dsw.command_stats() == dict(launches=0, steps=0, skipped=0)
    for x in (off.dsw, on.dsw, sol0, sol1):
        x.close()


class _DeviceBytes:
    """A device address as something torch.as_tensor takes"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(int(nbytes),), typestr="|u1", data=(int(ptr), False), version=2)


def test_the_device_pointers(hdsm):  # noqa: F811
    import torch
    prm = agile_params(10, max_rows_static=18)
    sol, rank = _one_rank(hdsm, prm)
    rank.dsw.set_commands(True)
    d_sp, d_pose = rank.dsw.commands_device()
    stream = torch.cuda.current_stream()
    for r in range(3):
        rank.dsw.round(stream=stream)
        stream.synchronize()
        step = rank.mirror.cfg.step_plan
        seen_sp = torch.as_tensor(_DeviceBytes(d_sp, N_ROB * step * 128), device="cuda").cpu().numpy().view(COMMAND).reshape(N_ROB, step)
        seen_pose = torch.as_tensor(_DeviceBytes(d_pose, N_ROB * 128), device="cuda").cpu().numpy().view(COMMAND)
        sp, pose = rank.dsw.commands()
        assert seen_sp.tobytes() == sp.tobytes() and seen_pose.tobytes() == pose.tobytes() and (pose["valid"] == 1).all(), r
        assert rank.dsw.commands_device() == (d_sp, d_pose)
    rank.dsw.close(), sol.close()


def test_k_command_uses_no_scratch_and_no_lds(tmp_path):
    assert_no_scratch_no_lds(tmp_path, "k_command")
