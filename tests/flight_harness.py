"""What the device-loop tests share: the library fixture, the host-mirror loop on the device solver, a circle flight with its
DeviceSwarm, the forest pair, the round-by-round comparison of device loop and host mirror, and the mirrored rank."""
import ctypes as C

import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.lib import call
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config


@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    return lib


def device_loop(hdsm, prm, cfg, n_rob, starts=None, goals=None, radius=None):
    from multi_agent_pkgs_amd import swarm
    sol = hdsm.Solver(prm, n_rob, n_rob)
    rcfg = agile_ref_config()

    def solve(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def ref_dev(ids, path, n_path, plans, has, vel_cap=None):
        full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    loop = swarm.SwarmLoop(prm, cfg, n_rob, solve=solve, radius=radius, reference=ref_dev, starts=starts, goals=goals)
    return sol, loop


def circle_flight(hdsm, prm, starts, goals, audit=False, groups=None, setup=None):
    """A flight on one rank with its DeviceSwarm: (solver, host-mirror loop, dswarm). setup(shard, rank), groups and the audit are
    set on the host mirror before the dswarm is made (what a DeviceSwarm takes over from its shard)."""
    sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), len(starts), starts=starts, goals=goals)
    if setup is not None:
        setup(loop.shard, 0)
    if groups is not None:
        loop.shard.set_groups(groups)
    if audit:
        loop.shard.set_audit(True, 1.0)
    return sol, loop, swarm.DeviceSwarm(loop.shard, sol)


def raw(dsw):
    """the plans buffer as it is (sentinels included)"""
    return dsw.download_raw()[0]


def agent_states(dsw, shard):
    """state_curr [n][9] of every agent, through a download into the host mirror"""
    dsw.download(states=True)
    ag = co.export_agents(shard)[0]
    return np.array([lc.arr(ag[a].state_curr, 9) for a in range(shard.n_local)])


def model():
    """The proposed model, as it stands: seed 7, wind (0.5, 0, 0), gust (2, 2, 1) m/s^2, jitter (0.01, 0.01, 0.005) m."""
    return sc.gust_model(7, (0.5, 0.0, 0.0), (2.0, 2.0, 1.0), (0.01, 0.01, 0.005))


def forest_pair(hdsm, n_rob, period, world_of=sc.inflate, clearance=None, seed=21):
    """Two host-mirror loops in the same forest, world_of(raw) as their world: ((sol, loop), (sol, loop))."""
    from multi_agent_pkgs_amd import swarm
    prm = agile_params(10, max_rows_static=18)
    raw, origin = sc.forest_for_circle(n_rob, seed=seed)
    world = world_of(raw)

    def make():
        sol, loop = device_loop(hdsm, prm, swarm.default_swarm_config(), n_rob)
        assert loop.set_world(world, origin) == 0
        loop.pmax = 49
        if clearance is not None:
            loop.shard.set_path_clearance(clearance)
        loop.shard.set_path_period(period)
        return sol, loop

    return make(), make()


PLAN_TOL = 1e-7   # plans of two flights that plan the same: the solver's staging order is not deterministic


def _compare(host, dsw, r):
    out = host.step()
    dsw.round()
    plans, has, status, failed = dsw.download(states=False)
    assert (has == host.has_plan).all(), r
    assert (status == out["status"]).all(), (r, status.tolist(), out["status"].tolist())
    assert np.abs(plans - host.plans_all).max() < PLAN_TOL, (r, float(np.abs(plans - host.plans_all).max()))


class MirroredRank:
    """One shard of a device flight with the host mirror that follows it: before a round the device's agent states go into the host
    mirror (hdsm_dswarm_download); behind it the round's reference, solver output and status — read back from the device's committed
    agents through a second shard — are handed to hdsm_swarm_set_reference / hdsm_swarm_commit of the mirror, which then looks from the
    same state_curr at the same reference point and commits the same record. The plans it publishes and the state it flew must be the
    device's, byte for byte, before a feature compares anything of its own (feature_round)."""

    def __init__(self, dsw, prm, cfg, starts, goals, n_fly=None):
        self.dsw, self.mirror, self.prm = dsw, dsw.shard, prm
        self.n = self.mirror.n_local
        self.n_fly = self.n if n_fly is None else n_fly
        self.post = swarm.SwarmShard(prm, cfg, self.mirror.n_rob, self.mirror.first_id, starts, goals)
        self.on = False

    def set_commands(self, on=True, yaw0=None):
        self.dsw.set_commands(on, yaw0=yaw0)
        self.mirror.set_commands(on, yaw0=yaw0)
        self.on = on

    def before_round(self):
        if self.n:
            self.dsw.download(states=True)
        self.pre = co.export_agents(self.mirror)[0]
        self.yaw = self.mirror.commands()[2] if self.on else None

    def after_round(self, tag):
        n, N, P = self.n, self.prm.n_hor, self.prm.poly_hor
        G = self.dsw.per * self.dsw.world_size
        plans, has, status, failed = np.zeros((G, N + 1, 9)), np.zeros(G, np.uint8), np.zeros(n, np.int32), C.c_int32(0)
        call("hdsm_dswarm_download", self.dsw.h, self.post.h if n else None, plans, has, status, C.byref(failed))
        if n == 0:
            return self.empty_round(tag)
        ag = co.export_agents(self.post)[0]
        ref_full = np.array([lc.arr(ag[k].traj_ref, co.MAXH + 1, 6)[:N + 1] for k in range(n)])
        self.mirror.set_reference(ref_full, np.array([ag[k].path_vel for k in range(n)]))
        out = dict(traj=np.array([lc.arr(ag[k].traj_curr, co.MAXH + 1, 9)[:N + 1] for k in range(n)]),
                   ctrl=np.array([lc.arr(ag[k].ctrl_curr, co.MAXH, 3)[:N] for k in range(n)]),
                   used=np.array([[ag[k].poly_used[j] for j in range(P)] for k in range(n)], np.uint8), status=status)
        mine, mine_has = self.mirror.commit(out)
        first, fly = self.mirror.first_id, self.n_fly
        assert mine[:fly].tobytes() == plans[first:first + fly].tobytes() and (mine_has[:fly] == has[first:first + fly]).all(), tag
        after = co.export_agents(self.mirror)[0]
        state = np.array([lc.arr(after[k].state_curr, 9) for k in range(n)])
        assert state[:fly].tobytes() == np.array([lc.arr(ag[k].state_curr, 9) for k in range(fly)]).tobytes(), tag     # (also the flown one)
        self.feature_round(tag, ref_full, out, after, state)

    def empty_round(self, tag):
        """what the feature checks on a rank without agents"""

    def feature_round(self, tag, ref_full, out, after, state):
        """what the feature adds: ref_full and out as the mirror committed them, the mirror's agents and their state_curr [n][9]
        after the commit"""
