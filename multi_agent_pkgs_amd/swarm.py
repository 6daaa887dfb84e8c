"""Closed-loop driver: shards of agents replanning in lock-step, one all-gather of the new plans per round.

Mirrors the sequencing of Agent::TrajPlanningIteration (agent_class.cpp:157-258) for a batch:

    prepare (host: corridor + reference)  ->  solve (device: planes + MIQP)  ->  commit (host: fallback,
    increment check, state advance)  ->  all-gather of the published plans (replaces the DDS all-to-all of
    agent_class.cpp:610-677)  ->  next round

The host-side steps live in libhdsm.so (csrc/swarm_host.cpp, include/hdsm_swarm.h). The solver is pluggable so
that the multi-process CPU tests can drive the same loop with the oracle standing in for the device.
"""
import ctypes as C

import numpy as np

from . import lib as _lib
from .lib import _f64, _i8, _i32, _stream, _u8, call
from .params import K_P_YAW, YAW_IDX, HdsmParams, MissionSummary, SwarmConfig  # noqa: F401  (SwarmConfig: the struct mirrors live in params.py)
from .scenarios import circle_formation, grid_formation, line_formation  # noqa: F401
from .scenarios import circle_scenario, lane_forest_scenario, lattice_scenario, repeat_scenario, shuttle_mission, square_mission  # noqa: F401  (scenario geometry lives in scenarios.py)


def default_swarm_config():
    cfg = SwarmConfig()
    _lib.load().hdsm_swarm_default_config(cfg)
    return cfg


def shard_range(n_rob, rank, world):
    """Contiguous id blocks, n_rob/world per rank."""
    per = (n_rob + world - 1) // world
    first = min(rank * per, n_rob)
    return first, min(per, n_rob - first)


def _box(values, lo):
    """An edit box as the world updates take it: (values int8 [bz][by][bx], lo (x, y, z), its dimensions (bx, by, bz))."""
    vals = _i8(values)
    assert vals.ndim == 3
    return vals, np.asarray(lo, dtype=np.int32), np.asarray(vals.shape[::-1], dtype=np.int32)


def _assign_call(fn, handle, n_local, group_start, slots, apply, setting):
    """hdsm_swarm_assign / hdsm_dswarm_assign: (slot_of int32 [n_local], stats lib.ASSIGN_STATS, one record per group)"""
    slots = _f64(slots).reshape(-1, 3)
    if slots.shape[0] != n_local:
        raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "assign: slots [n_local][3] expected")
    slot_of = np.full(n_local, -1, np.int32)
    stats = np.zeros(1 if group_start is None else len(group_start) - 1, _lib.ASSIGN_STATS)
    call(fn, handle, setting, slots, 1 if apply else 0, slot_of, stats)
    return slot_of, stats


def fly_formations(dsw, formations, mission_setting=None, max_rounds=400, check_every=4):
    """Fly a DeviceSwarm through formations (each [n_local][3], scenarios.*_formation) one after the other: assign(apply=False) on the
    states as they stand on the device, a one-waypoint mission on slots[slot_of] (an agent without a slot — the scripted tail — gets
    its own slot, which nobody flies), and fly() until every flown agent has arrived or max_rounds. mission_setting: params.Mission
    with n_wp = 1 (None: scenarios.mission_setting(1)). Returns (the summaries, the assignments slot_of) per formation. Built from
    the existing entries only."""
    from .scenarios import mission_setting as _mission_setting
    setting = _mission_setting(1) if mission_setting is None else mission_setting
    summaries, assignments = [], []
    for slots in formations:
        slots = _f64(slots).reshape(-1, 3)
        slot_of, _ = dsw.assign(slots, apply=False)
        take = np.where(slot_of >= 0, slot_of, np.arange(len(slot_of)))
        dsw.set_mission(setting, slots[take][:, None, :])
        rounds, summary = dsw.fly(max_rounds, check_every=check_every)
        summaries.append(dict(summary, rounds=rounds))
        assignments.append(slot_of)
    return summaries, assignments


class SwarmShard:
    """Host planner state of agents [first_id, first_id + n_local)."""

    def __init__(self, prm: HdsmParams, cfg: SwarmConfig, n_rob, first_id, starts, goals):
        self.lib = _lib.load()
        self.prm, self.cfg = prm.copy(), cfg
        self.n_rob, self.first_id = int(n_rob), int(first_id)
        starts, goals = _f64(starts), _f64(goals)
        self.n_local = starts.shape[0]
        self.h = C.c_void_p()
        self.world_shape = None
        call("hdsm_swarm_create", self.prm, self.cfg, self.n_rob, self.first_id, self.n_local, starts, goals, C.byref(self.h))
        N, P, RS, n = prm.n_hor, prm.poly_hor, prm.max_rows_static, self.n_local
        self.inp = dict(agent_id=np.zeros(n, np.int32), state=np.zeros((n, 9)), ref=np.zeros((n, N, 6)),
                        n_poly=np.zeros(n, np.int32), n_rows=np.zeros((n, P), np.int32),
                        A=np.zeros((n, P, RS, 3)), b=np.zeros((n, P, RS)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.hdsm_swarm_destroy(self.h)
            self.h = None

    def set_world(self, occupancy, origin=(0.0, 0.0, 0.0)):
        """occupancy int8 [nz][ny][nx] at cfg.voxel_size (>= 100 occupied, already inflated), or None for free space."""
        self.world_shape = None
        if occupancy is None:
            call("hdsm_swarm_set_world", self.h, None, np.zeros(3, np.int32), np.zeros(3))
        else:
            occ = _i8(occupancy)
            call("hdsm_swarm_set_world", self.h, occ, np.asarray(occ.shape[::-1], dtype=np.int32), np.asarray(origin, dtype=np.float64))
            self.world_shape = occ.shape  # (wz, wy, wx): what DeviceSwarm.download_world returns

    def update_world(self, values, lo):
        """hdsm_swarm_update_world: values int8 [bz][by][bx] replace the box of the processed world that starts at voxel lo (x, y, z).
        From the next corridor / path step on everything reads the new voxels; kept polyhedra are not checked again and paths
        adapt only through the path step."""
        call("hdsm_swarm_update_world", self.h, *_box(values, lo))

    def prepare_corridor(self):
        """GenerateSafeCorridor alone (hdsm_swarm_prepare_corridor): the reference's order when the reference trajectory is
        generated elsewhere — corridor from the previous reference first."""
        call("hdsm_swarm_prepare_corridor", self.h)

    def prepare(self, plans_all, has_plan):
        i = self.inp
        call("hdsm_swarm_prepare", self.h, _f64(plans_all), _u8(has_plan), i["agent_id"], i["state"], i["ref"], i["n_poly"], i["n_rows"],
             i["A"], i["b"])
        return i

    def reference_inputs(self, pmax=3):
        """Polyline each agent's reference will be sampled along this round (for hdsm_reference, f1)."""
        path = np.zeros((self.n_local, pmax, 3))
        n_path = np.zeros(self.n_local, np.int32)
        call("hdsm_swarm_reference_inputs_n", self.h, pmax, path, n_path)
        return path, n_path

    def vel_cap(self):
        """vel_cap for hdsm_reference: the voxel / potential-field term of ComputePathVelocity on the current world."""
        cap = np.zeros(self.n_local)
        call("hdsm_swarm_vel_cap", self.h, cap)
        return cap

    def route(self):
        """Global paths on the world given to set_world (hdsm_swarm_route); returns the number of agents without a route."""
        nf = C.c_int32(0)
        call("hdsm_swarm_route", self.h, C.byref(nf))
        return nf.value

    def set_paths(self, paths, n_path):
        paths = _f64(paths)
        call("hdsm_swarm_set_paths", self.h, paths, _i32(n_path), paths.shape[1])

    def get_paths(self, pmax=64):
        paths = np.zeros((self.n_local, pmax, 3))
        n_path = np.zeros(self.n_local, np.int32)
        call("hdsm_swarm_get_paths", self.h, pmax, paths, n_path)
        return paths, n_path

    def set_goals(self, goals):
        """GoalCallback (hdsm_swarm_set_goals): goals [n_local][3]; the agents whose goal changed plan a new path (csrc/path_core.h)
        at the start of the next round."""
        call("hdsm_swarm_set_goals", self.h, _f64(goals).reshape(self.n_local, 3))

    def set_path_clearance(self, search_rad):
        """hdsm_swarm_set_path_clearance: 0 (the default) the plain path step; non-zero: the distance-map planner in a tunnel of that
        radius round the descent (< 0: no tunnel) and ShortenDMPPath. The reference ships 1.8. Set before DeviceSwarm is made."""
        call("hdsm_swarm_set_path_clearance", self.h, search_rad)

    def set_path_period(self, period):
        """hdsm_swarm_set_path_period: every agent plans a new path every `period`-th round (0: never, the default)."""
        call("hdsm_swarm_set_path_period", self.h, int(period))

    def replan_paths(self):
        """hdsm_swarm_replan_paths: every local agent plans a new path now; returns the number that failed (kept their path)."""
        nf = C.c_int32(0)
        call("hdsm_swarm_replan_paths", self.h, C.byref(nf))
        return nf.value

    def path_errors(self):
        """(agents whose last path step failed, status per agent)."""
        codes = np.zeros(self.n_local, np.int32)
        return self.lib.hdsm_swarm_path_errors(self.h, codes), codes

    def corridor_errors(self):
        codes = np.zeros(self.n_local, np.int32)
        return self.lib.hdsm_swarm_corridor_errors(self.h, codes), codes

    def set_reference(self, ref_full, path_vel):
        call("hdsm_swarm_set_reference", self.h, _f64(ref_full), _f64(path_vel))

    def commit(self, out):
        plans_local = np.zeros((self.n_local, self.prm.n_hor + 1, 9))
        has_local = np.zeros(self.n_local, np.uint8)
        call("hdsm_swarm_commit", self.h, _f64(out["traj"]), _f64(out["ctrl"]), _u8(out["used"]), _i32(out["status"]), plans_local, has_local)
        return plans_local, has_local

    def set_groups(self, group_start=None):
        """hdsm_swarm_set_groups: group_start [n_groups + 1] partitions the ids [0, n_rob) into contiguous ranges; an agent's
        neighbours are the agents of its own range (the host reference generation and the audit; a DeviceSwarm made from this shard
        takes the partition over and sets it on its solver). None: one group."""
        gs = _i32([] if group_start is None else group_start)
        if gs.size < 2:
            call("hdsm_swarm_set_groups", self.h, 0, None)
        else:
            call("hdsm_swarm_set_groups", self.h, gs.size - 1, gs)
        self.group_start = None if gs.size < 2 else gs.copy()

    def set_audit(self, on=True, sep_warn=1.0):
        """hdsm_swarm_set_audit: the flight audit of the host mirror (csrc/audit_core.h). The flight record starts when it is first
        switched on; a round counts as close when its separation ratio is below sep_warn. SwarmLoop.step audits every round while
        it is on, and a DeviceSwarm made from this shard takes the setting and the record over."""
        call("hdsm_swarm_set_audit", self.h, 1 if on else 0, sep_warn)

    @property
    def audit_on(self):
        """hdsm_swarm_get_audit: whether the mirror audits — asked of the library, so that a setting brought back from a device
        loop (DeviceSwarm.download) counts like one made here."""
        on = C.c_int32(0)
        call("hdsm_swarm_get_audit", self.h, C.byref(on), None)
        return bool(on.value)

    def audit(self, plans_all, has_plan):
        """hdsm_swarm_audit: one round into the flight record — the records all agents published this round (after the gather)."""
        plans_all, has_plan = _f64(plans_all), _u8(has_plan)
        if plans_all.shape != (self.n_rob, self.prm.n_hor + 1, 9) or has_plan.shape != (self.n_rob,):
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "audit: plans_all [n_rob][n_hor+1][9] and has_plan [n_rob] expected")
        call("hdsm_swarm_audit", self.h, plans_all, has_plan)

    def flight_report(self):
        """hdsm_swarm_flight_report: the flight record per local agent (lib.FLIGHT_REPORT); an error if the audit was never on."""
        rep = np.zeros(self.n_local, _lib.FLIGHT_REPORT)
        call("hdsm_swarm_flight_report", self.h, rep)
        return rep

    # ---- imperfect tracking (include/hdsm_swarm.h) ----
    def set_tracking(self, model=None):
        """hdsm_swarm_set_tracking: from the next commit on every agent with a plan flies lib.track_states of traj_curr[step_plan]
        under the model (params.Tracking, scenarios.gust_model) instead of arriving where it planned; the tracking round starts at
        0. None: off, the records are kept. Not carried into a DeviceSwarm: set it there too."""
        call("hdsm_swarm_set_tracking", self.h, model)

    def set_states(self, states, mask=None):
        """hdsm_swarm_set_states: states [n_local][9] measured outside (a simulator, odometry) replace state_curr of the masked agents
        (mask [n_local], None: all); a row with a non-finite value is skipped."""
        call("hdsm_swarm_set_states", self.h, _f64(states).reshape(self.n_local, 9), None if mask is None else _u8(mask).reshape(self.n_local))

    def track_records(self):
        """hdsm_swarm_track_records: the tracking record per local agent (lib.TRACK_RECORD; tracking_summary folds them)."""
        rec = np.zeros(self.n_local, _lib.TRACK_RECORD)
        call("hdsm_swarm_track_records", self.h, rec)
        return rec

    # ---- commands for the vehicle (include/hdsm_swarm.h) ----
    def set_commands(self, on=True, yaw_idx=YAW_IDX, k_p_yaw=K_P_YAW, yaw0=None):
        """hdsm_swarm_set_commands: from the next commit on every agent's yaw follows reference point yaw_idx (ComputeYawAngle) and the
        commit leaves the setpoints of the interval about to be flown and the pose the round ends in (commands()). yaw0 [n_local]: the
        yaw to start from (None: zeros). on=False: off, the yaw kept. A DeviceSwarm made from this shard takes setting and yaw over."""
        call("hdsm_swarm_set_commands", self.h, 1 if on else 0, int(yaw_idx), float(k_p_yaw), None if yaw0 is None else _f64(yaw0).reshape(self.n_local))

    def commands(self):
        """hdsm_swarm_commands: (setpoint [n_local][step_plan], pose [n_local] of lib.COMMAND, yaw [n_local]) of the last commit."""
        sp, pose = np.zeros((self.n_local, self.cfg.step_plan), _lib.COMMAND), np.zeros(self.n_local, _lib.COMMAND)
        yaw = np.zeros(self.n_local)
        call("hdsm_swarm_commands", self.h, sp, pose, yaw)
        return sp, pose, yaw

    # ---- a vehicle in the loop (include/hdsm_swarm.h) ----
    def set_vehicle(self, model=None):
        """hdsm_swarm_set_vehicle: from the next commit on every agent's vehicle (params.Vehicle, scenarios.crazyflie_vehicle) flies the
        round's setpoints sub-step by sub-step behind the command step, and state_curr, the track records and the poses take what it
        flew. Needs set_commands on and no tracking model. A switch-on seats every vehicle on state_curr and the command yaw. None:
        off. A DeviceSwarm made from this shard takes setting and vehicles over."""
        call("hdsm_swarm_set_vehicle", self.h, model)

    def vehicle_states(self):
        """hdsm_swarm_vehicle_states: the vehicle per local agent (lib.VEHICLE_STATE)."""
        vs = np.zeros(self.n_local, _lib.VEHICLE_STATE)
        call("hdsm_swarm_vehicle_states", self.h, vs)
        return vs

    # ---- missions (include/hdsm_swarm.h) ----
    def set_mission(self, setting=None, waypoints=None, count=None):
        """hdsm_swarm_set_mission: setting (params.Mission, scenarios.mission_setting), waypoints [n_local][n_wp][3], count [n_local]
        (None: every agent visits all). The records are reset, every agent's goal becomes its waypoint 0 and is due at the next round;
        from then on every commit judges the state flown (lib.mission_step). None: off, goals and records stay. A DeviceSwarm made
        from this shard takes setting, table, records and mission round over."""
        if setting is None:
            call("hdsm_swarm_set_mission", self.h, None, None, None)
            return
        waypoints, count = _lib.mission_table(waypoints, count)
        if waypoints.shape[:2] != (self.n_local, setting.n_wp):
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "set_mission: waypoints [n_local][setting.n_wp][3] expected")
        call("hdsm_swarm_set_mission", self.h, setting, waypoints, count)

    def mission_records(self):
        """hdsm_swarm_mission_records: the mission record per local agent (lib.MISSION_RECORD)."""
        rec = np.zeros(self.n_local, _lib.MISSION_RECORD)
        call("hdsm_swarm_mission_records", self.h, rec)
        return rec

    def mission_summary(self):
        """hdsm_swarm_mission_summary: the shard's summary of the mission round judged last, as a dict (params.MissionSummary)."""
        s = MissionSummary()
        call("hdsm_swarm_mission_summary", self.h, C.byref(s))
        return s.as_dict()

    def mission_due(self):
        """hdsm_swarm_mission_due: (due uint8 [n_local]: the agents that plan a path at the next round, goals [n_local][3])."""
        due, goals = np.zeros(self.n_local, np.uint8), np.zeros((self.n_local, 3))
        call("hdsm_swarm_mission_due", self.h, due, goals)
        return due, goals

    # ---- formations (include/hdsm_swarm.h) ----
    def assign(self, slots, apply=True, setting=None):
        """hdsm_swarm_assign: which agent takes which of slots [n_local][3] (lib.assign on state_curr, in the shard's neighbour
        groups). apply: the permuted slots become the goals, exactly as set_goals would set them (refused while a mission is on).
        Returns (slot_of int32 [n_local], stats: one lib.ASSIGN_STATS record per group). One rank only."""
        return _assign_call("hdsm_swarm_assign", self.h, self.n_local, getattr(self, "group_start", None), slots, apply, setting)

    def state(self):
        pos = np.zeros((self.n_local, 3))
        dist = np.zeros(self.n_local)
        nfail = np.zeros(self.n_local, np.int32)
        self.lib.hdsm_swarm_state(self.h, pos, dist, nfail)
        return pos, dist, nfail


class SwarmLoop:
    """One rank of the lock-step loop. `solve(inputs, plans_all, has_plan) -> out dict` is the device solver
    (or, in CPU tests, the oracle); `allgather(local_array) -> full array` exchanges the shards."""

    def __init__(self, prm, cfg, n_rob, rank=0, world=1, solve=None, allgather=None, radius=None, reference=None,
                 starts=None, goals=None):
        """reference(agent_id, path, n_path, plans_all, has_plan) -> (ref_full, path_vel): when given, the reference
        trajectory comes from it (the device kernel of row f1, or the oracle) instead of the host code.
        starts / goals [n_rob][3]: explicit scenario (default: the circular exchange)."""
        self.prm, self.n_rob, self.rank, self.world = prm, n_rob, rank, world
        self.reference = reference
        self.has_world = False
        self.pmax = 3  # points of the reference polyline handed to `reference` (16 after route())
        if starts is None:
            starts, goals = circle_scenario(n_rob, radius)
        starts, goals = np.asarray(starts, dtype=np.float64), np.asarray(goals, dtype=np.float64)
        self.first, self.n_local = shard_range(n_rob, rank, world)
        sl = slice(self.first, self.first + self.n_local)
        self.shard = SwarmShard(prm, cfg, n_rob, self.first, starts[sl], goals[sl])
        self.solve, self.allgather = solve, allgather
        N = prm.n_hor
        self.plans_all = np.zeros((n_rob, N + 1, 9))
        self.has_plan = np.zeros(n_rob, np.uint8)
        self.round_idx = 0

    def set_world(self, occupancy, origin, route=True):
        """Occupied world for the corridor generator (f2) and, with route=True, global paths from the built-in router."""
        self.shard.set_world(occupancy, origin)
        self.has_world = occupancy is not None
        if route:
            failed = self.shard.route()
            self.pmax = 32
            return failed
        return 0

    def update_world(self, values, lo):
        """A map update between two rounds (SwarmShard.update_world)."""
        self.shard.update_world(values, lo)

    def step(self, record=None):
        if self.reference is not None:
            self.shard.prepare_corridor()  # AC:165 before AC:171
            path, n_path = self.shard.reference_inputs(self.pmax)
            ids = np.arange(self.first, self.first + self.n_local, dtype=np.int32)
            ref_full, pv = self.reference(ids, path, n_path, self.plans_all, self.has_plan, **({"vel_cap": self.shard.vel_cap()} if self.has_world else {}))
            self.shard.set_reference(ref_full, pv)
        inputs = self.shard.prepare(self.plans_all, self.has_plan)
        if record is not None:
            record.append(dict({k: v.copy() for k, v in inputs.items()}, plans=self.plans_all.copy(),
                               has_plan=self.has_plan.copy()))
        out = self.solve(inputs, self.plans_all, self.has_plan)
        plans_local, has_local = self.shard.commit(out)
        if self.world > 1:
            per = (self.n_rob + self.world - 1) // self.world
            pad = per - self.n_local  # equal-size shards for the collective
            pl = np.concatenate([plans_local, np.zeros((pad,) + plans_local.shape[1:])]) if pad else plans_local.copy()
            hl = np.concatenate([has_local, np.zeros(pad, np.uint8)]) if pad else has_local
            # ONE collective per round: the has_plan flag travels inside the record (first entry NaN = no plan), exactly like
            # hdsm_publish_device / hdsm_exchange_device do on the device
            pl[hl == 0, 0, 0] = np.nan
            full = self.allgather(pl)[: self.n_rob]
            self.has_plan = (~np.isnan(full[:, 0, 0])).astype(np.uint8)
            full[self.has_plan == 0, 0, 0] = 0.0
            self.plans_all = full
        else:
            self.plans_all, self.has_plan = plans_local, has_local
        if self.shard.audit_on:
            self.shard.audit(self.plans_all, self.has_plan)
        self.round_idx += 1
        return out


def poly_octa3d(grid, seed, n_it=42, res=0.3, mark=-1, origin=(0.0, 0.0, 0.0), max_rows=18, shape_aware=False):
    """Convex voxel decomposition around `seed` (hdsm_poly_octa3d = GetPolyOcta3D of the reference; shape_aware:
    hdsm_poly_octa3d_new = GetPolyOcta3DNew).
    grid: int8 [nz][ny][nx] (x fastest), < 100 free, >= 100 occupied; modified in place (taken voxels = mark).
    Returns rows [k][4] = (n, n . p), n . x <= n . p."""
    grid = _i8(grid)
    nz, ny, nx = grid.shape
    rows = np.zeros((max_rows, 4))
    n = C.c_int32(0)
    call("hdsm_poly_octa3d_new" if shape_aware else "hdsm_poly_octa3d", np.asarray(seed, dtype=np.int32), grid,
         np.asarray([nx, ny, nz], dtype=np.int32), int(n_it), res, int(mark), np.asarray(origin, dtype=np.float64), rows, int(max_rows),
         C.byref(n))
    return rows[: n.value].copy(), grid


def torch_allgather(group=None):
    """all-gather of a numpy shard through torch.distributed (gloo on CPU, RCCL via 'nccl' on GPUs)."""
    import torch
    import torch.distributed as dist

    def fn(local):
        t = torch.from_numpy(np.ascontiguousarray(local))
        if dist.get_backend(group) == "nccl":
            t = t.cuda()
        world = dist.get_world_size(group)
        full = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(full, t, group=group)
        return full.cpu().numpy()

    return fn


class DeviceSwarm:
    """The device-resident closed loop of one shard (hdsm_dswarm_*): corridor -> reference -> replan -> commit -> exchange on one
    stream. Built from a SwarmShard that has been set up (world, paths) and possibly flown, and an hdsm Solver."""

    def __init__(self, shard, solver, world_size=1, device=0):
        self.lib, self.shard, self.solver = _lib.load(), shard, solver
        self.h = C.c_void_p()
        self.world_size = int(world_size)
        call("hdsm_dswarm_create", shard.h, solver.h, device, world_size, C.byref(self.h))
        self.per = (shard.n_rob + self.world_size - 1) // self.world_size
        gs = getattr(shard, "group_start", None)
        self.n_groups = 1 if gs is None else len(gs) - 1   # (the partition is taken from the shard when the dswarm is made)

    def upload_plans(self, plans_all, has_plan):
        call("hdsm_dswarm_upload_plans", self.h, _f64(plans_all), _u8(has_plan))

    def round(self, comm=None, stream=None):
        call("hdsm_dswarm_round", self.h, comm.h if comm is not None else None, _stream(stream))

    def download(self, states=True):
        """Synchronises; returns (plans_all, has_plan, status of the last round, instances without solution so far) and, with
        states=True, copies the agent states back into the host mirror."""
        N, G = self.shard.prm.n_hor, self.per * self.world_size
        plans = np.zeros((G, N + 1, 9))
        has = np.zeros(G, np.uint8)
        status = np.zeros(self.shard.n_local, np.int32)
        failed = C.c_int32(0)
        call("hdsm_dswarm_download", self.h, self.shard.h if states else None, plans, has, status, C.byref(failed))
        return plans, has, status, failed.value

    def download_raw(self):
        """hdsm_dswarm_download_raw: (plans buffer [per * world_size][N+1][9] as it is, sentinels included; send buffer
        [per][N+1][9]). Synchronises the device."""
        N = self.shard.prm.n_hor
        plans, send = np.zeros((self.per * self.world_size, N + 1, 9)), np.zeros((self.per, N + 1, 9))
        call("hdsm_dswarm_download_raw", self.h, plans, send)
        return plans, send

    PHASES =("k_corridor", "k_vel_cap", "hdsm_reference_device", "k_keep_free", "hdsm_replan_device", "k_commit", "exchange")

    def set_phase_timing(self, on=True):
        """hdsm_dswarm_set_phase_timing: HIP events between the launches of the following rounds (see phase_ms)."""
        call("hdsm_dswarm_set_phase_timing", self.h, 1 if on else 0)

    def phase_ms(self):
        """Milliseconds of the last timed round per phase (PHASES order); synchronises with that round."""
        ms = np.zeros(7, np.float32)
        call("hdsm_dswarm_last_phase_ms", self.h, ms)
        return dict(zip(self.PHASES, [float(x) for x in ms]))

    def _counters(self, fn, n):
        out = np.zeros(n, np.int64)
        call(fn, self.h, out)
        return [int(x) for x in out]

    def cache_stats(self):
        """hdsm_dswarm_cache_stats: what the device corridor's polyhedron cache did since the dswarm was created."""
        asked, same, interior, on = self._counters("hdsm_dswarm_cache_stats", 4)
        return {"asked": asked, "hits_same_grid": same, "hits_interior": interior, "cache_on": bool(on)}

    def set_goals(self, goals):
        """hdsm_dswarm_set_goals: goals [n_local][3]; the changed agents plan a new path at the next round (on the device)."""
        call("hdsm_dswarm_set_goals", self.h, _f64(goals).reshape(self.shard.n_local, 3))

    def path_stats(self):
        """hdsm_dswarm_path_stats: agents planned by k_path, of them failed, and launches since the dswarm was created."""
        return dict(zip(("planned", "failed", "launches"), self._counters("hdsm_dswarm_path_stats", 3)))

    def _ms(self, fn):
        ms = C.c_float(0.0)
        call(fn, self.h, C.byref(ms))
        return float(ms.value)

    def last_path_ms(self):
        """hdsm_dswarm_last_path_ms: milliseconds of k_path in the last timed round (0.0 if it planned nothing)."""
        return self._ms("hdsm_dswarm_last_path_ms")

    # ---- map updates in flight (include/hdsm_swarm.h, ABI 1.7) ----
    def update_world(self, values, lo):
        """hdsm_dswarm_update_world: PROCESSED values int8 [bz][by][bx] into the box of the device world that starts at voxel lo
        (x, y, z); the cache entries that looked at the box are dropped. Synchronises."""
        call("hdsm_dswarm_update_world", self.h, *_box(values, lo))

    def set_raw_world(self, map_cfg, raw_full):
        """hdsm_dswarm_set_raw_world: a RAW grid int8 [wz][wy][wx] (-1, 0, 100) becomes resident, the device world its
        hdsm_map_preprocess with map_cfg (params.MapConfig); every cache entry is dropped. Synchronises."""
        raw = _i8(raw_full)
        if raw.shape != self.shard.world_shape:
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "set_raw_world: a grid of the world's dimensions expected")
        call("hdsm_dswarm_set_raw_world", self.h, map_cfg, raw)

    def update_world_raw(self, raw_values, lo, stream=None):
        """hdsm_dswarm_update_world_raw: RAW values int8 [bz][by][bx] into the resident raw grid at voxel lo, the region pre-processing
        into the device world, the cache entries that looked at the written box W dropped. A numpy array: copied in, synchronises.
        A torch device tensor (int8, contiguous): hdsm_dswarm_update_world_raw_device, asynchronous on `stream` — which must be the
        stream the rounds run on; keep the tensor alive until the stream has passed the edit."""
        if hasattr(raw_values, "data_ptr"):
            assert raw_values.is_cuda and raw_values.is_contiguous() and raw_values.dim() == 3 and raw_values.element_size() == 1
            lo, bdim = np.asarray(lo, dtype=np.int32), np.asarray(tuple(raw_values.shape)[::-1], dtype=np.int32)
            call("hdsm_dswarm_update_world_raw_device", self.h, raw_values, lo, bdim, _stream(stream))
        else:
            call("hdsm_dswarm_update_world_raw", self.h, *_box(raw_values, lo))

    def download_world(self):
        """hdsm_dswarm_download_world: the processed device world, int8 [wz][wy][wx]. Synchronises."""
        if self.shard.world_shape is None:
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "download_world: the shard has no world")
        world = np.zeros(self.shard.world_shape, np.int8)
        call("hdsm_dswarm_download_world", self.h, world)
        return world

    def world_stats(self):
        """hdsm_dswarm_world_stats: map updates applied, voxels they wrote, cache entries dropped, whether a raw world is resident."""
        updates, voxels, dropped, raw = self._counters("hdsm_dswarm_world_stats", 4)
        return {"updates": updates, "voxels": voxels, "dropped": dropped, "raw_resident": bool(raw)}

    # ---- link faults (include/hdsm_swarm.h) ----
    def set_links(self, fate=None, time_aware=True):
        """hdsm_dswarm_set_links: fate int8 [n_rounds][n_rob] (scenarios.link_table), read cyclically — entry (q mod n_rounds, k) is
        the fate of the record agent k publishes in link round q: < 0 lost for everyone, d in 0..7 it arrives d rounds late. Link
        round 0 is the next round. time_aware: a stale record is read advanced by its age (else as it is, like the reference).
        None (or an empty table) turns links off. Per sender: every receiver sees the same thing. Synchronises."""
        if fate is None or np.size(fate) == 0:
            call("hdsm_dswarm_set_links", self.h, 0, None, 0)
            return
        fate = _i8(fate)
        if fate.ndim != 2 or fate.shape[1] != self.shard.n_rob:
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "set_links: a table [n_rounds][n_rob] expected")
        call("hdsm_dswarm_set_links", self.h, fate.shape[0], fate, 1 if time_aware else 0)

    def link_stats(self):
        """hdsm_dswarm_link_stats: link rounds since set_links, records delivered into views, broadcasts lost, the largest age (in
        rounds) any agent's slot reached. Synchronises."""
        return dict(zip(("rounds", "delivered", "lost", "max_age"), self._counters("hdsm_dswarm_link_stats", 4)))

    def download_seen(self):
        """hdsm_dswarm_download_seen: the view the next round reads — (seen_raw [G][N+1][9] with the sentinel of a slot without a plan,
        seen_has [G], seen_round [G] (-1: the view of the set_links call), shift [G]), G = world_size * per. Synchronises."""
        N, G = self.shard.prm.n_hor, self.per * self.world_size
        seen, has = np.zeros((G, N + 1, 9)), np.zeros(G, np.uint8)
        seen_round, shift = np.zeros(G, np.int32), np.zeros(G, np.int32)
        call("hdsm_dswarm_download_seen", self.h, seen, has, seen_round, shift)
        return seen, has, seen_round, shift

    # ---- scripted agents (include/hdsm_swarm.h) ----
    def set_script(self, knots, predict=0):
        """hdsm_dswarm_set_script: the LAST n_script agents of the shard follow the tracks knots [n_script][n_knots][4] of (t, x, y, z)
        (scenarios.hold_track / line_track; tau = 0 is the start of the next round) instead of being planned for, and publish the
        records of lib.script_records; predict=1: beyond the round's end the record continues at constant velocity. n_script may
        stay (new tracks) or grow (a dropout), never shrink. Synchronises."""
        knots = _lib._tracks(knots)
        call("hdsm_dswarm_set_script", self.h, knots.shape[0], knots.shape[1], knots, int(predict))

    def script_stats(self):
        """hdsm_dswarm_script_stats: script rounds since the last set_script, scripted agents, launches of k_script."""
        return dict(zip(("rounds", "n_script", "launches"), self._counters("hdsm_dswarm_script_stats", 3)))

    # ---- imperfect tracking (include/hdsm_swarm.h) ----
    def set_tracking(self, model=None):
        """hdsm_dswarm_set_tracking: from the next round on k_track, right behind k_commit, makes every flown agent with a plan fly
        lib.track_states of traj_curr[step_plan] under the model (params.Tracking, scenarios.gust_model); the published records stay
        the plans, the history holds the flown states. The tracking round starts at 0. None: off, records kept. Synchronises."""
        call("hdsm_dswarm_set_tracking", self.h, model)

    def set_states(self, states, mask=None, stream=None):
        """States [n_local][9] measured outside replace state_curr of the masked flown agents (mask [n_local] of uint8, None: all; a row
        with a non-finite value is skipped) before the next round. A numpy array: hdsm_dswarm_set_states, copied in, synchronises.
        Anything with data_ptr() (a float64 device tensor; the mask a uint8 one): hdsm_dswarm_set_states_device, asynchronous on
        `stream` — which must be the stream the rounds run on; keep the tensors alive until the stream has passed the call."""
        n = self.shard.n_local
        if hasattr(states, "data_ptr"):
            assert states.is_cuda and states.numel() == n * 9 and (mask is None or (mask.is_cuda and mask.numel() == n))
            call("hdsm_dswarm_set_states_device", self.h, states, mask, _stream(stream))
        else:
            call("hdsm_dswarm_set_states", self.h, _f64(states).reshape(n, 9), None if mask is None else _u8(mask).reshape(n))

    def track_records(self):
        """hdsm_dswarm_track_records: the tracking record per local agent (lib.TRACK_RECORD). Synchronises."""
        rec = np.zeros(self.shard.n_local, _lib.TRACK_RECORD)
        call("hdsm_dswarm_track_records", self.h, rec)
        return rec

    def track_stats(self):
        """hdsm_dswarm_track_stats: tracking rounds since the model was set, launches of k_track's model form and of its external form."""
        return dict(zip(("rounds", "model_launches", "external_launches"), self._counters("hdsm_dswarm_track_stats", 3)))

    def plans_device(self):
        """hdsm_dswarm_plans_device: the device addresses (plans buffer [world * per][N+1][9] of float64, flags [world * per] of uint8),
        read-only and valid for the dswarm's life — what a simulator on the same GPU reads to know what to execute."""
        plans, has = C.c_void_p(), C.c_void_p()
        call("hdsm_dswarm_plans_device", self.h, C.byref(plans), C.byref(has))
        return plans.value, has.value

    # ---- commands for the vehicle (include/hdsm_swarm.h) ----
    def set_commands(self, on=True, yaw_idx=YAW_IDX, k_p_yaw=K_P_YAW, yaw0=None):
        """hdsm_dswarm_set_commands: from the next round on k_command, the last launch behind k_commit, steps every flown agent's yaw
        towards reference point yaw_idx and writes the setpoints of the interval about to be flown and the pose the round ends in.
        yaw0 [n_local]: the yaw to start from (None: zeros). on=False: off, yaw and records kept. Commands never steer: the plans
        are what they are without them. Synchronises."""
        n = self.shard.n_local
        call("hdsm_dswarm_set_commands", self.h, 1 if on else 0, int(yaw_idx), float(k_p_yaw), None if yaw0 is None else _f64(yaw0).reshape(n))

    def commands(self):
        """hdsm_dswarm_commands: (setpoint [n_local][step_plan], pose [n_local]) of lib.COMMAND as the last round left them; setpoint[k][0]
        is what planner_crazyswarm_bridge sends as FullState, its yaw field 11 of Trajectory.msg. Synchronises."""
        n = self.shard.n_local
        sp, pose = np.zeros((n, self.shard.cfg.step_plan), _lib.COMMAND), np.zeros(n, _lib.COMMAND)
        call("hdsm_dswarm_commands", self.h, sp, pose)
        return sp, pose

    def commands_device(self):
        """hdsm_dswarm_commands_device: the device addresses of (setpoint [n_local][step_plan], pose [n_local]), 128-byte hdsm_command
        records, valid for the dswarm's life and written on the rounds' stream — what a vehicle model on the same GPU reads."""
        sp, pose = C.c_void_p(), C.c_void_p()
        call("hdsm_dswarm_commands_device", self.h, C.byref(sp), C.byref(pose))
        return sp.value, pose.value

    def command_stats(self):
        """hdsm_dswarm_command_stats: launches of k_command, agent-rounds with a yaw step taken, agent-rounds skipped (the reference point
        closer than sqrt(0.1) m, or missing). Synchronises once commands were on."""
        return dict(zip(("launches", "steps", "skipped"), self._counters("hdsm_dswarm_command_stats", 3)))

    # ---- a vehicle in the loop (include/hdsm_swarm.h) ----
    def set_vehicle(self, model=None):
        """hdsm_dswarm_set_vehicle: from the next round on k_vehicle, right behind k_command, flies every flown agent's vehicle
        (params.Vehicle, scenarios.crazyflie_vehicle) against the round's setpoints — step_plan * n_sub controller evaluations and RK4
        steps — and state_curr, the history, the track records and the poses take what it flew. Needs set_commands on and no tracking
        model. A switch-on seats every vehicle on state_curr and the yaw. None: off. Synchronises."""
        call("hdsm_dswarm_set_vehicle", self.h, model)

    def vehicle_states(self):
        """hdsm_dswarm_vehicle_states: the vehicle per local agent (lib.VEHICLE_STATE). Synchronises."""
        vs = np.zeros(self.shard.n_local, _lib.VEHICLE_STATE)
        call("hdsm_dswarm_vehicle_states", self.h, vs)
        return vs

    def vehicle_states_device(self):
        """hdsm_dswarm_vehicle_states_device: the device address of the vehicle states [n_local], 128-byte hdsm_vehicle_state records,
        valid for the dswarm's life and written on the rounds' stream."""
        p = C.c_void_p()
        call("hdsm_dswarm_vehicle_states_device", self.h, C.byref(p))
        return p.value

    def vehicle_stats(self):
        """hdsm_dswarm_vehicle_stats: launches of k_vehicle, agent-rounds flown, vehicles re-seated (an end state that was not finite),
        sub-steps with the thrust clamped, sub-steps with a body rate clamped. Synchronises once a vehicle was on."""
        return dict(zip(("launches", "flown", "reseated", "thrust_clamped", "rate_clamped"), self._counters("hdsm_dswarm_vehicle_stats", 5)))

    # ---- missions (include/hdsm_swarm.h) ----
    def set_mission(self, setting=None, waypoints=None, count=None):
        """hdsm_dswarm_set_mission: setting (params.Mission, scenarios.mission_setting), waypoints [n_local][n_wp][3], count [n_local]
        (None: all). The records are reset, every flown agent's goal becomes its waypoint 0 and is due at the next round; from then
        on k_mission, the last launch behind k_commit, judges what was flown, writes an arrived agent's next goal and flags it for
        the next round's path step — on the device. None: off, goals and records stay. While a mission is on set_goals is refused.
        Synchronises."""
        if setting is None:
            call("hdsm_dswarm_set_mission", self.h, None, None, None)
            return
        waypoints, count = _lib.mission_table(waypoints, count)
        if waypoints.shape[:2] != (self.shard.n_local, setting.n_wp):
            raise _lib.HdsmError(_lib.HDSM_ERR_BAD_ARG, "set_mission: waypoints [n_local][setting.n_wp][3] expected")
        call("hdsm_dswarm_set_mission", self.h, setting, waypoints, count)

    def mission_records(self):
        """hdsm_dswarm_mission_records: the mission record per local agent (lib.MISSION_RECORD). Synchronises."""
        rec = np.zeros(self.shard.n_local, _lib.MISSION_RECORD)
        call("hdsm_dswarm_mission_records", self.h, rec)
        return rec

    def mission_summary(self):
        """hdsm_dswarm_mission_summary: the shard's summary of the mission round judged last, as a dict. Synchronises."""
        s = MissionSummary()
        call("hdsm_dswarm_mission_summary", self.h, C.byref(s))
        return s.as_dict()

    def mission_due(self):
        """hdsm_dswarm_mission_due: (the pending due flags uint8 [n_local], the goal buffer [n_local][3]). Synchronises."""
        due, goals = np.zeros(self.shard.n_local, np.uint8), np.zeros((self.shard.n_local, 3))
        call("hdsm_dswarm_mission_due", self.h, due, goals)
        return due, goals

    def mission_stats(self):
        """hdsm_dswarm_mission_stats: launches of k_mission, path launches sized on the device, agents those launches planned."""
        return dict(zip(("launches", "path_launches", "planned"), self._counters("hdsm_dswarm_mission_stats", 3)))

    def mission_groups(self):
        """hdsm_dswarm_mission_groups: the mission per neighbour group over the group's local flown agents (lib.MISSION_GROUP; one
        record for the whole shard without a partition). Synchronises."""
        out = np.zeros(self.n_groups, _lib.MISSION_GROUP)
        call("hdsm_dswarm_mission_groups", self.h, out)
        return out

    def fly(self, max_rounds, check_every=4, stop_on_stall=False, stream=None):
        """hdsm_dswarm_fly: rounds without the caller until every flown agent is done (stop_on_stall: done or stalled), polled every
        check_every rounds, max_rounds at the most. Returns (rounds flown, the last summary polled as a dict). One rank only."""
        rounds, last = C.c_int32(0), MissionSummary()
        call("hdsm_dswarm_fly", self.h, _stream(stream), int(max_rounds), int(check_every), 1 if stop_on_stall else 0, C.byref(rounds), C.byref(last))
        return rounds.value, last.as_dict()

    # ---- formations (include/hdsm_swarm.h) ----
    def assign(self, slots, apply=True, setting=None):
        """hdsm_dswarm_assign: which flown agent takes which of slots [n_local][3] — k_assign on state_curr where it lives, one
        workgroup per neighbour group; no state is downloaded. The scripted tail keeps -1. apply: the permuted slots become the goals
        through set_goals (refused while a mission is on). Returns (slot_of int32 [n_local], stats: one lib.ASSIGN_STATS record per
        group). A set-up call: it synchronises. One rank only."""
        return _assign_call("hdsm_dswarm_assign", self.h, self.shard.n_local, getattr(self.shard, "group_start", None) if self.n_groups > 1 else None,
                            slots, apply, setting)

    def set_audit(self, on=True, sep_warn=1.0):
        """hdsm_dswarm_set_audit: the flight audit at the end of every round (k_audit_pack, k_audit, k_audit_track); synchronises."""
        call("hdsm_dswarm_set_audit", self.h, 1 if on else 0, sep_warn)

    def flight_report(self):
        """hdsm_dswarm_flight_report: the flight record per local agent (lib.FLIGHT_REPORT); an error if the audit was never on."""
        rep = np.zeros(self.shard.n_local, _lib.FLIGHT_REPORT)
        call("hdsm_dswarm_flight_report", self.h, rep)
        return rep

    def group_report(self):
        """hdsm_dswarm_group_report: the flight per group over the group's local agents (lib.GROUP_REPORT; one record for the whole
        swarm without a partition) — last statuses, failures, distance to the goal and the fold of the flight records. Synchronises."""
        out = np.zeros(self.n_groups, _lib.GROUP_REPORT)
        call("hdsm_dswarm_group_report", self.h, out)
        return out

    def last_audit_round(self):
        """hdsm_dswarm_last_audit_round: what the last round's audit found per local agent (lib.AUDIT_ROUND)."""
        out = np.zeros(self.shard.n_local, _lib.AUDIT_ROUND)
        call("hdsm_dswarm_last_audit_round", self.h, out)
        return out

    def last_audit_ms(self):
        """hdsm_dswarm_last_audit_ms: milliseconds of the audit's launches in the last timed round (0.0 if it launched none)."""
        return self._ms("hdsm_dswarm_last_audit_ms")

    def set_history(self, capacity_rounds):
        """hdsm_dswarm_set_history: record state_curr of every local agent after each round's commit, for capacity_rounds rounds
        (then recording stops and the lost rounds are counted); 0 switches it off. Starts an empty history."""
        call("hdsm_dswarm_set_history", self.h, int(capacity_rounds))
        self._hist_cap = int(capacity_rounds)

    def history(self, mirror=True):
        """hdsm_dswarm_download_history: (hist [n_rounds][n_local][9], rounds dropped). mirror=True also appends every round not yet
        delivered to the planner records of the host mirror (state_hist_<id>.csv of hdsm_swarm_shutdown), once."""
        cap = getattr(self, "_hist_cap", 0)
        hist = np.zeros((max(cap, 1), self.shard.n_local, 9))
        n, dropped = C.c_int32(0), C.c_int32(0)
        call("hdsm_dswarm_download_history", self.h, self.shard.h if mirror else None, hist, cap, C.byref(n), C.byref(dropped))
        return hist[: n.value].copy(), dropped.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hdsm_dswarm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalRanks:
    """A sharded swarm flown by ONE process (hdsm_comm_create_local / hdsm_dswarm_round_ranks, ABI 1.9): the `world` blocks of
    shard_range as host mirrors, one solver handle and one DeviceSwarm per rank — on devices[r], default all on device 0 — and a
    local communicator group; round() flies one replan round of all ranks with one call. setup(shard, rank), if given, is called on
    every host mirror before its dswarm is made (world, paths, groups, audit: what a DeviceSwarm takes over from its shard)."""

    def __init__(self, prm, cfg, n_rob, world, starts=None, goals=None, radius=None, devices=None, setup=None):
        self.lib = _lib.load()
        self.n_rob, self.world = int(n_rob), int(world)
        self.per = (self.n_rob + self.world - 1) // self.world
        self.devices = [0] * self.world if devices is None else [int(d) for d in devices]
        assert len(self.devices) == self.world
        if starts is None:
            starts, goals = circle_scenario(n_rob, radius)
        starts, goals = np.asarray(starts, dtype=np.float64), np.asarray(goals, dtype=np.float64)
        self.shards, self.solvers, self.dswarms = [], [], []
        self._comms = (C.c_void_p * self.world)()
        for r in range(self.world):
            first, n_local = shard_range(self.n_rob, r, self.world)
            shard = SwarmShard(prm, cfg, self.n_rob, first, starts[first:first + n_local], goals[first:first + n_local])
            if setup is not None:
                setup(shard, r)
            self.shards.append(shard)
            self.solvers.append(_lib.Solver(prm, self.per, self.world * self.per, device=self.devices[r]))
        handles = (C.c_void_p * self.world)(*[s.h.value for s in self.solvers])
        call("hdsm_comm_create_local", self.world, handles, self._comms)
        for r in range(self.world):
            self.dswarms.append(DeviceSwarm(self.shards[r], self.solvers[r], world_size=self.world, device=self.devices[r]))
        self._dsw = (C.c_void_p * self.world)(*[d.h.value for d in self.dswarms])

    @property
    def comms(self):
        """The hdsm_comm of every rank (addresses)."""
        return [self._comms[r] for r in range(self.world)]

    def round(self, streams=None):
        """hdsm_dswarm_round_ranks: one round of every rank; streams: one torch stream per rank (None entries, or None: the default)."""
        st = (C.c_void_p * self.world)(*[_stream(s) for s in (streams or [None] * self.world)])
        call("hdsm_dswarm_round_ranks", self.world, self._dsw, self._comms, st)

    def download_raw(self, rank):
        """DeviceSwarm.download_raw of one rank: (plans buffer [world * per][N+1][9], send buffer [per][N+1][9])."""
        return self.dswarms[rank].download_raw()

    def close(self):
        for d in self.dswarms:
            d.close()
        self.dswarms = []
        for r in range(self.world):
            if self._comms[r]:
                self.lib.hdsm_comm_destroy(self._comms[r])
                self._comms[r] = None
        for s in self.solvers:
            s.close()
        self.solvers = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def flight_summary(reports, first_id=0):
    """Folds per-agent flight records (lib.FLIGHT_REPORT, of one shard or concatenated in id order starting at first_id) into a swarm
    summary: sigma_min (the smallest separation ratio flown, None without a pair) with both ids, the sub-step and the agent's audited
    round; close_rounds (agent-rounds below sep_warn: a close pair counts once for each of its agents); the totals; the mean
    potential under the positions flown, pot_sum / positions; the mean and the largest speed."""
    rep = np.asarray(reports)
    out = dict(agents=int(rep.size), rounds=int(rep["rounds"].max()) if rep.size else 0, positions=int(rep["positions"].sum()),
               sigma_min=None, sigma_min_agent=-1, sigma_min_partner=-1, sigma_min_substep=0, sigma_min_round=-1,
               close_rounds=int(rep["close_rounds"].sum()), occupied=int(rep["occupied"].sum()), unknown=int(rep["unknown"].sum()),
               crossed=int(rep["crossed"].sum()), pot_sum=int(rep["pot_sum"].sum()), dist=float(rep["dist"].sum()))
    out["mean_potential"] = out["pot_sum"] / out["positions"] if out["positions"] else 0.0
    flown = rep["rounds"] > 0
    out["mean_speed"] = float((rep["speed_sum"][flown] / rep["rounds"][flown]).mean()) if flown.any() else 0.0
    out["max_speed"] = float(rep["speed_max"].max()) if rep.size else 0.0
    paired = np.nonzero(rep["sep_partner"] >= 0)[0]
    if paired.size:
        k = paired[np.lexsort((paired, rep["sep2_min"][paired]))[0]]     # smallest sep2_min, then the lower id
        out.update(sigma_min=float(np.sqrt(rep["sep2_min"][k])), sigma_min_agent=int(first_id + k), sigma_min_partner=int(rep["sep_partner"][k]),
                   sigma_min_substep=int(rep["sep_substep"][k]), sigma_min_round=int(rep["sep_round"][k]))
    return out


def tracking_summary(records):
    """Folds per-agent tracking records (lib.TRACK_RECORD, of one shard or concatenated) into the three figures of the reference's
    planner_crazyswarm_bridge/scripts/tracking_error.py over all samples (model rounds + states taken from outside): the mean, the
    standard deviation (population, as numpy.std) and the maximum of the distance between the planned and the flown position; with
    them the number of samples and the largest velocity difference."""
    rec = np.asarray(records)
    n = int(rec["rounds"].sum() + rec["external"].sum())
    if n == 0:
        return dict(samples=0, mean=0.0, std=0.0, max=0.0, dvel_max=0.0)
    mean = float(rec["dist_sum"].sum()) / n
    var = max(float(rec["dist_sq_sum"].sum()) / n - mean * mean, 0.0)
    return dict(samples=n, mean=mean, std=float(np.sqrt(var)), max=float(rec["dist_max"].max()), dvel_max=float(rec["dvel_max"].max()))


def flown_records(hist, starts):
    """From a state history hist [rounds][n][9] (DeviceSwarm.history; starts [n][3] or [n][9]: where the agents stood before round 0)
    the two-state records [rounds][n][2][9] = (state before the round, state after it) that lib.flight_audit_host / flight_audit_batch
    accept with n_hor = 1 and step_plan = 1: the motion actually FLOWN judged with the audit that exists, where the device audit
    judges the published plans. The audit joins the two states by a straight segment: for step_plan > 1 that is the chord of the
    flown interval, not its sub-steps."""
    hist = np.asarray(hist, dtype=np.float64)
    starts = np.asarray(starts, dtype=np.float64)
    first = np.zeros((1,) + hist.shape[1:])
    first[0, :, :starts.shape[1]] = starts
    before = np.concatenate([first, hist[:-1]])
    return np.ascontiguousarray(np.stack([before, hist], axis=2))
