"""ctypes binding of libhdsm.so (the C ABI of include/hdsm.h, hdsm_swarm.h and hdsm_stats.h).

The headers are the only place a signature is written: load() parses the three of them once (parse_declarations) and sets
``restype`` and ``argtypes`` on every function they declare, so a call takes Python numbers, numpy arrays, torch tensors and the
struct mirrors of params.py as they are. A ``T*`` parameter (ArrayPtr) refuses an array of another dtype, a non-contiguous one
and a tensor of another element size with ``ctypes.ArgumentError`` before the library is entered. call() is the one call path:
a non-zero return code becomes an :class:`HdsmError` carrying the text of the function's family (ERROR_TEXT).

There is deliberately no fallback: if the shared library has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C multi_agent_pkgs_amd/csrc``) importing the library raises,
and creating a solver on a machine without a HIP device raises :class:`HdsmError` (HDSM_ERR_NO_DEVICE).
"""
import ctypes as C
import os
import re

import numpy as np

from .params import (AssignSetting, AssignStats, Command, HdsmParams, MapConfig, Mission, MissionSummary, RefConfig, SwarmConfig, Tracking,
                     TrackRecord, Vehicle, VehicleState)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("HDSM_LIBRARY") or os.path.join(_HERE, "libhdsm.so")  # (HDSM_LIBRARY: a development build, e.g. -DCD_PROFILE)
INCLUDE = os.path.join(_HERE, os.pardir, "include")
HEADERS = ("hdsm.h", "hdsm_swarm.h", "hdsm_stats.h")

HDSM_OK, HDSM_ERR_BAD_ARG, HDSM_ERR_NO_DEVICE, HDSM_ERR_DEVICE, HDSM_ERR_CAPACITY, HDSM_ERR_COMM = 0, -1, -2, -3, -4, -5
HDSM_FLAG_NODE_LIMIT, HDSM_FLAG_ITER_LIMIT, HDSM_FLAG_TIME_LIMIT, HDSM_FLAG_STAGING_OVERFLOW = 1, 2, 4, 8
HDSM_COMM_ID_BYTES = 128

# ---- the records of the flight audit (include/hdsm_swarm.h, csrc/audit_core.h) ----
AUDIT_ROUND = np.dtype([("sep2", "<f8"), ("partner", "<i4"), ("substep", "<i4"), ("occupied", "<i4"), ("unknown", "<i4"),
                        ("crossed", "<i4"), ("pot", "<i4"), ("dist", "<f8"), ("speed", "<f8")])          # hdsm_audit_round
FLIGHT_REPORT = np.dtype([("rounds", "<i8"), ("positions", "<i8"), ("sep2_min", "<f8"), ("sep_partner", "<i4"), ("sep_substep", "<i4"),
                          ("sep_round", "<i8"), ("close_rounds", "<i8"), ("occupied", "<i8"), ("unknown", "<i8"), ("crossed", "<i8"),
                          ("pot_sum", "<i8"), ("dist", "<f8"), ("speed_sum", "<f8"), ("speed_max", "<f8")])  # hdsm_flight_report
GROUP_REPORT = np.dtype([("first", "<i4"), ("count", "<i4"), ("n_local", "<i4"), ("no_solution_last", "<i4"), ("failed_total", "<i8"),
                         ("dist_goal_max", "<f8"), ("rounds", "<i8"), ("positions", "<i8"), ("close_rounds", "<i8"), ("occupied", "<i8"),
                         ("unknown", "<i8"), ("crossed", "<i8"), ("pot_sum", "<i8"), ("sep2_min", "<f8"), ("sep_agent", "<i4"),
                         ("sep_partner", "<i4"), ("sep_substep", "<i4"), ("reserved0", "<i4"), ("sep_round", "<i8"),
                         ("speed_max", "<f8")])                                                            # hdsm_group_report
TRACK_RECORD = np.dtype([("rounds", "<i8"), ("external", "<i8"), ("dist_sum", "<f8"), ("dist_sq_sum", "<f8"), ("dist_max", "<f8"),
                         ("dvel_max", "<f8")])                                                             # hdsm_track_record
COMMAND = np.dtype([("pos", "<f8", 3), ("vel", "<f8", 3), ("acc", "<f8", 3), ("quat", "<f8", 4), ("yaw", "<f8"), ("valid", "<i4"), ("pad", "<i4"),
                    ("reserved0", "<f8")])                                                                 # hdsm_command
VEHICLE_STATE = np.dtype([("pos", "<f8", 3), ("vel", "<f8", 3), ("quat", "<f8", 4), ("omega", "<f8", 3), ("thrust", "<f8"), ("yaw_cmd", "<f8"),
                          ("reserved0", "<f8")])                                                           # hdsm_vehicle_state
VEHICLE = np.dtype([("n_sub", "<i4"), ("feed", "<i4"), ("acc_from", "<i4"), ("pad", "<i4"), ("kp", "<f8", 3), ("kv", "<f8", 3), ("k_att", "<f8", 3),
                    ("tau_rate", "<f8"), ("tau_thrust", "<f8"), ("thrust_min", "<f8"), ("thrust_max", "<f8"), ("rate_max", "<f8", 3),
                    ("drag", "<f8", 3), ("seed", "<u8"), ("wind", "<f8", 3), ("gust", "<f8", 3)])            # hdsm_vehicle
MISSION_RECORD = np.dtype([("wp", "<i4"), ("done", "<i4"), ("dwell", "<i4"), ("stalled", "<i4"), ("laps", "<i4"), ("stall_events", "<i4"),
                           ("since", "<i4"), ("arrivals", "<i4"), ("done_round", "<i8"), ("last_arrival_round", "<i8"), ("dist", "<f8"),
                           ("best_dist", "<f8"), ("arrive_round", "<i4", 16)])                            # hdsm_mission_record
MISSION_GROUP = np.dtype([("first", "<i4"), ("count", "<i4"), ("n_local", "<i4"), ("done", "<i4"), ("stalled", "<i4"), ("laps_min", "<i4"),
                          ("laps_max", "<i4"), ("reserved0", "<i4"), ("arrivals", "<i8"), ("makespan", "<i8")])    # hdsm_mission_group
MISSION_MAX_WP = 16  # HDSM_MISSION_MAX_WP
ASSIGN_STATS = np.dtype([("first", "<i4"), ("count", "<i4"), ("active", "<i4"), ("status", "<i4"), ("phases", "<i4"), ("reserved0", "<i4"),
                         ("iters", "<i8"), ("bids", "<i8"), ("cost", "<i8")])                              # hdsm_assign_stats
ASSIGN_MAX = 1024  # HDSM_ASSIGN_MAX
assert ASSIGN_STATS.itemsize == 48 == C.sizeof(AssignStats) and C.sizeof(AssignSetting) == 16
assert MISSION_RECORD.itemsize == 128 and MISSION_GROUP.itemsize == 48 and C.sizeof(Mission) == 48 and C.sizeof(MissionSummary) == 40
assert COMMAND.itemsize == 128 == C.sizeof(Command)
assert VEHICLE_STATE.itemsize == 128 == C.sizeof(VehicleState) and VEHICLE.itemsize == 224 == C.sizeof(Vehicle)
assert AUDIT_ROUND.itemsize == 48 and FLIGHT_REPORT.itemsize == 104 and GROUP_REPORT.itemsize == 128
assert TRACK_RECORD.itemsize == 48 == C.sizeof(TrackRecord) and C.sizeof(Tracking) == 80


class HdsmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hdsm error {code}: {msg}")
        self.code = code


class ArrayPtr:
    """The argtype of a `T*` parameter: a C-contiguous numpy array of exactly T, a contiguous tensor (anything with data_ptr())
    of T's size, or whatever c_void_p takes (None, byref(...), ctypes arrays and pointers, an address)."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        self.itemsize = self.dtype.itemsize

    def from_param(self, a):
        if isinstance(a, np.ndarray):
            if a.dtype != self.dtype or not a.flags.c_contiguous:
                raise TypeError(f"a C-contiguous {self.dtype} array expected, not {a.dtype}{'' if a.flags.c_contiguous else ', not contiguous'}")
            return C.c_void_p(a.ctypes.data)
        data_ptr = getattr(a, "data_ptr", None)
        if data_ptr is not None:
            if a.element_size() != self.itemsize or not a.is_contiguous():
                raise TypeError(f"a contiguous tensor of {self.itemsize}-byte elements expected, not {a.dtype}, stride {tuple(a.stride())}")
            return C.c_void_p(data_ptr())
        return C.c_void_p.from_param(a)


CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t, "void*": C.c_void_p,
          "void**": C.POINTER(C.c_void_p), "char*": C.c_char_p}
CTYPES.update({t + "*": ArrayPtr(d) for t, d in (("double", np.float64), ("int32_t", np.int32), ("int8_t", np.int8), ("uint8_t", np.uint8),
                                                  ("uint32_t", np.uint32), ("int64_t", np.int64), ("float", np.float32),
                                                  ("hdsm_audit_round", AUDIT_ROUND), ("hdsm_flight_report", FLIGHT_REPORT),
                                                  ("hdsm_group_report", GROUP_REPORT), ("hdsm_track_record", TRACK_RECORD), ("hdsm_command", COMMAND),
                                                  ("hdsm_vehicle_state", VEHICLE_STATE), ("hdsm_mission_record", MISSION_RECORD),
                                                  ("hdsm_mission_group", MISSION_GROUP), ("hdsm_assign_stats", ASSIGN_STATS))})
CTYPES.update({t + "*": C.POINTER(s) for t, s in (("hdsm_params", HdsmParams), ("hdsm_ref_config", RefConfig), ("hdsm_map_config", MapConfig),
                                                  ("hdsm_swarm_config", SwarmConfig), ("hdsm_tracking", Tracking), ("hdsm_vehicle", Vehicle),
                                                  ("hdsm_mission", Mission), ("hdsm_mission_summary", MissionSummary),
                                                  ("hdsm_assign_setting", AssignSetting))})


def parse_declarations(text):
    """{name: (restype, argtypes)} of every `<ret> hdsm_name(<args>);` in the text of a header. `T x[3]` is `T*`, `T* const* x` (an
    array of pointers the callee only reads) is `T**`; a C type that CTYPES does not know raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def ctype(decl, fn, ret=False):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)\s*(?:const\s*(\*)\s*)?(?:\w+\s*(\[\w*\])?)?", decl.strip())
        key = m and m.group(1) + m.group(2) + (m.group(3) or "") + ("*" if m.group(4) else "")
        if ret and key == "void":
            return None
        if key not in CTYPES:
            raise TypeError(f"{fn}: no ctypes mapping for the C type '{' '.join(decl.split())}'")
        return CTYPES[key]

    out = {}
    for ret, fn, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(hdsm_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[fn] = (ctype(ret, fn, ret=True), [ctype(a, fn) for a in args])
    return out


def _header_declarations():
    sigs = {}
    for h in HEADERS:
        with open(os.path.join(INCLUDE, h)) as f:
            sigs.update(parse_declarations(f.read()))
    return sigs


SIGNATURES = _header_declarations()
EXPORTS = tuple(SIGNATURES)

# The text of an HdsmError, by prefix of the function's name (the first match): the family's *_last_error function, or None for
# the functions that report their own name.
ERROR_TEXT = (("hdsm_dswarm_upload_plans", None), ("hdsm_dswarm_", "hdsm_dswarm_last_error"), ("hdsm_map_", "hdsm_map_last_error"),
              ("hdsm_poly_octa3d_batch", "hdsm_corridor_last_error"), ("hdsm_poly_octa3d", None), ("hdsm_swarm_", None),
              ("hdsm_local_path_", None), ("hdsm_flight_audit_", None), ("hdsm_link_", None), ("hdsm_script_", None), ("hdsm_track_", None),
              ("hdsm_command_", None), ("hdsm_vehicle_", None), ("hdsm_mission_", None), ("hdsm_assign_", None),
              ("hdsm_", "hdsm_last_error"))

_lib = None


def load():
    """Load libhdsm.so; raises if it is missing (no silent fallback). Every function the headers declare gets its signature."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        # One ROCm runtime per process. libhdsm.so links /opt/rocm's libamdhip64 / librccl; PyTorch bundles its own copies under
        # the SAME sonames, and whichever is mapped first serves both. A process that also uses torch (device tensors, streams)
        # must let torch map its copies first, or torch no longer finds the GPU ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(SO_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


def call(name, *args):
    """The one call path: libhdsm's `name` on args; a non-zero return code raises HdsmError with the text ERROR_TEXT gives."""
    lib = _lib or load()
    rc = getattr(lib, name)(*args)
    if rc:
        err = next(e for prefix, e in ERROR_TEXT if name.startswith(prefix))
        raise HdsmError(rc, getattr(lib, err)().decode() if err else name)


def _p(a, t):
    """A ctypes pointer to the data of a numpy array, for callers of the raw functions (the tests); the argtypes take it as they
    take the array itself."""
    return a.ctypes.data_as(C.POINTER(t))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _i8(a):
    return np.ascontiguousarray(a, dtype=np.int8)


def _stream(stream):
    """The hipStream_t of a torch stream (None: the default stream)."""
    return stream.cuda_stream if stream is not None else None


def _world(world):
    """(world int8 [wz][wy][wx], its dimensions (wx, wy, wz)) as the batch entry points take them; (None, None) is free space."""
    if world is None:
        return None, None
    world = _i8(world)
    return world, np.asarray(world.shape[::-1], dtype=np.int32)


def host_register(arr):
    """hdsm_host_register on a C-contiguous numpy array that the caller keeps alive and reuses every round (page-locked,
    mapped: DMA without staging; output arrays of replan() are then written by the device). Undo with host_unregister()."""
    assert arr.flags["C_CONTIGUOUS"] and arr.nbytes > 0
    call("hdsm_host_register", arr.ctypes.data, arr.nbytes)
    return arr


def host_unregister(arr):
    call("hdsm_host_unregister", arr.ctypes.data)


class Solver:
    """One hdsm handle (= the persistent GRBModel of one planner thread, but batched)."""

    def __init__(self, prm: HdsmParams, max_instances: int, n_rob_max: int, device: int = 0):
        self.lib = load()
        self.prm = prm.copy()
        self.max_instances, self.n_rob_max, self.device = int(max_instances), int(n_rob_max), int(device)
        self.h = C.c_void_p()
        call("hdsm_create", self.prm, self.max_instances, self.n_rob_max, self.device, C.byref(self.h))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hdsm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _out(self, n_inst):
        N, P = self.prm.n_hor, self.prm.poly_hor
        return dict(traj=np.zeros((n_inst, N + 1, 9)), ctrl=np.zeros((n_inst, N, 3)), used=np.zeros((n_inst, P), dtype=np.uint8),
                    status=np.zeros(n_inst, dtype=np.int32), obj=np.zeros(n_inst))

    # ---- host-pointer entry point (PCIe inclusive) -------------------------------------------------------
    def replan(self, agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan, out=None, stats=True):
        agent_id, n_poly, n_rows = _i32(agent_id), _i32(n_poly), _i32(n_rows)
        state, ref, A, b, plans, has_plan = _f64(state), _f64(ref), _f64(A), _f64(b), _f64(plans), _u8(has_plan)
        n_inst, n_rob = state.shape[0], plans.shape[0]
        if out is None:
            out = self._out(n_inst)
        call("hdsm_replan", self.h, n_inst, n_rob, agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan,
             out["traj"], out["ctrl"], out["used"], out["status"], out["obj"])
        if stats:
            out.update(self.last_stats(n_inst))
        return out

    # ---- device-pointer entry point: torch tensors (already resident in HBM), async on `stream` ---------
    def replan_device(self, agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan, traj, ctrl, used,
                      status, obj, stream=None):
        """All arguments are CUDA(HIP) torch tensors with the dtypes/layouts of include/hdsm.h."""
        n_inst, n_rob = state.shape[0], plans.shape[0]
        for t in (agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan, traj, ctrl, used, status, obj):
            assert t.is_cuda  # (contiguity and element size: the argtypes)
        call("hdsm_replan_device", self.h, n_inst, n_rob, agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan, traj, ctrl, used,
             status, obj, _stream(stream))

    def solve(self, state, ref, n_poly, n_rows, A, b, out=None):
        """Level 1 (hdsm_solve): fully formed per-step polyhedra poly_const_final_vec_[N][<=P]."""
        state, ref, A, b = _f64(state), _f64(ref), _f64(A), _f64(b)
        n_poly, n_rows = _i32(n_poly), _i32(n_rows)
        n_inst, r_max = state.shape[0], A.shape[3]
        if out is None:
            out = self._out(n_inst)
        call("hdsm_solve", self.h, n_inst, r_max, state, ref, n_poly, n_rows, A, b, out["traj"], out["ctrl"], out["used"], out["status"],
             out["obj"])
        return out

    def reference(self, cfg, agent_id, path, n_path, plans, has_plan, vel_cap=None):
        """Next row f1 (hdsm_reference): path_vel + sampled reference for every instance. path [n_inst][pmax][3]."""
        N = self.prm.n_hor
        agent_id, n_path = _i32(agent_id), _i32(n_path)
        path, plans, has_plan = _f64(path), _f64(plans), _u8(has_plan)
        n_inst, pmax, n_rob = path.shape[0], path.shape[1], plans.shape[0]
        ref_full, ref, pv = np.zeros((n_inst, N + 1, 6)), np.zeros((n_inst, N, 6)), np.zeros(n_inst)
        cap = _f64(vel_cap) if vel_cap is not None else None
        call("hdsm_reference", self.h, cfg, n_inst, n_rob, agent_id, path, n_path, pmax, cap, plans, has_plan, ref_full, ref, pv)
        return ref_full, ref, pv

    def reference_device(self, cfg, agent_id, path, n_path, plans, has_plan, ref_full, ref, path_vel, vel_cap=None,
                         stream=None):
        """hdsm_reference_device on CUDA/HIP torch tensors (asynchronous on `stream`)."""
        n_inst, pmax, n_rob = path.shape[0], path.shape[1], plans.shape[0]
        call("hdsm_reference_device", self.h, cfg, n_inst, n_rob, agent_id, path, n_path, pmax, vel_cap, plans, has_plan, ref_full, ref,
             path_vel, _stream(stream))

    def tasc_planes(self, agent_id, state, plans, has_plan):
        N = self.prm.n_hor
        agent_id, state, plans, has_plan = _i32(agent_id), _f64(state), _f64(plans), _u8(has_plan)
        n_inst, n_rob = state.shape[0], plans.shape[0]
        planes = np.zeros((n_inst, N, n_rob, 4))
        call("hdsm_tasc_planes", self.h, n_inst, n_rob, agent_id, state, plans, has_plan, planes)
        return planes

    def set_groups(self, group_start=None):
        """hdsm_set_groups: group_start [n_groups + 1] partitions the agent ids into contiguous ranges (0 first, strictly increasing,
        the last entry = the number of agents); from then on an agent's neighbours are the agents of its own range, in replan*,
        reference* and tasc_planes. None (or an empty list): one group, as without the call. Synchronises the handle."""
        gs = _i32([] if group_start is None else group_start)
        if gs.size < 2:
            call("hdsm_set_groups", self.h, 0, None)
        else:
            call("hdsm_set_groups", self.h, gs.size - 1, gs)

    # ---- stale plans (include/hdsm.h) ----
    def set_plan_shift(self, shift=None):
        """hdsm_set_plan_shift: shift [n_rob] >= 0 — every instance but k's own reads record k advanced by shift[k] steps with its
        last state held (values above n_hor behave as n_hor). None (or an empty list) clears it. Honoured by replan*, reference* and
        tasc_planes. Synchronises the handle."""
        sh = _i32([] if shift is None else shift)
        call("hdsm_set_plan_shift", self.h, sh.size, sh if sh.size else None)

    def set_plan_shift_device(self, d_shift=None):
        """hdsm_set_plan_shift_device: a BORROWED int32 device tensor [n_rob], read by every later launch; None clears it. Keep the
        tensor alive while it is set."""
        call("hdsm_set_plan_shift_device", self.h, d_shift)

    def set_own_plans_device(self, d_own_plans=None, d_own_has=None):
        """hdsm_set_own_plans_device: BORROWED device tensors in the layouts of plans / has_plan; the instance of agent a takes its
        own previous plan and flag from there instead of plans[a] / has_plan[a] (d_own_has None: the flag stays has_plan[a]). None
        clears the override. Keep the tensors alive while they are set."""
        call("hdsm_set_own_plans_device", self.h, d_own_plans, d_own_has)

    def reset_warm_start(self):
        call("hdsm_reset_warm_start", self.h)

    def last_sweep_stats(self, n_inst):
        st = dict(sphere_records=np.zeros(n_inst, dtype=np.int32), pairs=np.zeros(n_inst, dtype=np.int32),
                  flags=np.zeros(n_inst, dtype=np.uint32))
        call("hdsm_last_sweep_stats", self.h, n_inst, st["sphere_records"], st["pairs"], st["flags"])
        return st

    def set_kernel_timing(self, on=True):
        call("hdsm_set_kernel_timing", self.h, 1 if on else 0)

    def last_kernel_ms(self):
        ms = C.c_float(0.0)
        call("hdsm_last_kernel_ms", self.h, C.byref(ms))
        return float(ms.value)

    def last_stats(self, n_inst):
        st = {k: np.zeros(n_inst, dtype=np.int32) for k in ("qp_iters", "nodes", "sweeps", "cand")}
        call("hdsm_last_stats", self.h, n_inst, st["qp_iters"], st["nodes"], st["sweeps"], st["cand"])
        return st


def comm_unique_id():
    """hdsm_comm_unique_id (rank 0): 128 opaque bytes the launcher hands to every rank."""
    buf = (C.c_uint8 * HDSM_COMM_ID_BYTES)()
    call("hdsm_comm_unique_id", buf)
    return bytes(buf)


class Comm:
    """One RCCL communicator of the per-round plan exchange (hdsm_comm_* / hdsm_exchange_device)."""

    def __init__(self, solver, unique_id, rank, world):
        self.lib = load()
        self.h = C.c_void_p()
        buf = (C.c_uint8 * HDSM_COMM_ID_BYTES).from_buffer_copy(unique_id)
        call("hdsm_comm_create", solver.h, buf, int(rank), int(world), C.byref(self.h))
        r, w = C.c_int32(-1), C.c_int32(-1)
        call("hdsm_comm_info", self.h, C.byref(r), C.byref(w))
        self.rank, self.world, self.solver = r.value, w.value, solver

    def publish_device(self, traj, has_local, plans_local, n_local=None, stream=None):
        per = plans_local.shape[0]
        n_local = per if n_local is None else int(n_local)
        call("hdsm_publish_device", self.solver.h, per, n_local, traj, has_local, plans_local, _stream(stream))

    def exchange_device(self, plans_local, plans_all, has_all, stream=None):
        """ONE all-gather: plans_local [per][N+1][9] of every rank -> plans_all [world*per][N+1][9], has_all [world*per]."""
        per = plans_local.shape[0]
        assert plans_all.shape[0] == per * self.world and has_all.shape[0] == per * self.world
        call("hdsm_exchange_device", self.h, per, plans_local, plans_all, has_all, _stream(stream))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hdsm_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_preprocess(cfg, grids, device=0):
    """hdsm_map_preprocess: grids int8 [n][nz][ny][nx] (-1 unknown, 0 free, 100 occupied) -> same shape, after
    SetUncertainToUnknown, InflateObstacles and CreatePotentialField (next row f4). Runs on the GPU."""
    g = _i8(grids)
    assert g.ndim == 4
    out = np.empty_like(g)
    call("hdsm_map_preprocess", device, cfg, g.shape[0], np.asarray(g.shape[:0:-1], dtype=np.int32), g, out)
    return out


def map_preprocess_device(cfg, d_in, d_out, d_scratch, stream=None, device=0):
    """Device-pointer variant on torch tensors: d_in/d_out int8 [n][nz][ny][nx], d_scratch uint8 with >= 2 * d_in.numel()."""
    dim = np.asarray(tuple(d_in.shape)[:0:-1], dtype=np.int32)
    assert d_scratch.numel() >= 2 * d_in.numel() and d_in.is_contiguous() and d_out.is_contiguous()
    call("hdsm_map_preprocess_device", device, cfg, d_in.shape[0], dim, d_in, d_out, d_scratch.data_ptr(), _stream(stream))


def map_region_extent(cfg, dim, lo, bdim):
    """hdsm_map_region_extent: for an edit box lo .. lo + bdim (x, y, z voxels) of a raw grid of dimensions dim (nx, ny, nz), the
    box W the processed grid can change in and the working box the stages run on: (write_lo, write_dim, work_lo, work_dim), each an
    int32 array of three. Host arithmetic only."""
    out = [np.zeros(3, np.int32) for _ in range(4)]
    call("hdsm_map_region_extent", cfg, _i32(dim), _i32(lo), _i32(bdim), *out)
    return tuple(out)


def map_preprocess_region(cfg, raw_full, out_full, lo, bdim, device=0):
    """hdsm_map_preprocess_region: raw_full int8 [nz][ny][nx] is the raw grid AFTER an edit inside the box lo .. lo + bdim (x, y, z),
    out_full the processed grid of BEFORE it. Returns the processed grid of after it (a new array): the nine passes run on the
    working box only, and only W is written. Runs on the GPU."""
    raw = _i8(raw_full)
    out = np.array(out_full, dtype=np.int8, order="C", copy=True)
    assert raw.ndim == 3 and out.shape == raw.shape
    call("hdsm_map_preprocess_region", device, cfg, np.asarray(raw.shape[::-1], dtype=np.int32), raw, out, _i32(lo), _i32(bdim))
    return out


def poly_octa3d_batch(world, ldim, off, ground_k, seed, variant, origin, n_it=42, res=0.3, max_rows=32, device=0, wave=False):
    """hdsm_poly_octa3d_batch (row f2 on the device): world int8 [wz][wy][wx]; off/seed [n][3], ground_k/variant [n], origin [n][3].
    Returns rows [n][max_rows][4], n_rows [n], rc [n], cells [n]. wave=True: hdsm_poly_octa3d_batch_wave (one wavefront per seed)."""
    world, wdim = _world(world)
    off, seed = _i32(off), _i32(seed)
    n = off.shape[0]
    rows = np.zeros((n, max_rows, 4))
    n_rows, rc, cells = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    call("hdsm_poly_octa3d_batch_wave" if wave else "hdsm_poly_octa3d_batch", device, n, world, wdim, np.asarray(ldim, dtype=np.int32), off,
         _i32(ground_k), seed, _i32(variant), _f64(origin), n_it, res, rows, max_rows, n_rows, rc, cells)
    return rows, n_rows, rc, cells


PATH_PTS = 48  # points of a global path (csrc/swarm_core.h)


def _local_path(fn, lead, world, ldim, off, ground_k, origin, start, goal, res, pmax, search_rad=None):
    off = _i32(off)
    n = off.shape[0]
    world, wdim = _world(world)
    paths = np.zeros((n, pmax, 3))
    n_path, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    cost, n_raw = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    extra_in, extra_out = ((), ()) if search_rad is None else ((search_rad,), (cost, n_raw))
    call(fn, *lead, n, world, wdim, np.asarray(ldim, dtype=np.int32), off, _i32(ground_k), _f64(origin), _f64(start), _f64(goal), res,
         *extra_in, pmax, paths, n_path, status, *extra_out)
    return (paths, n_path, status) if search_rad is None else (paths, n_path, status, cost, n_raw)


def local_path_batch(world, ldim, off, ground_k, origin, start, goal, res=0.3, pmax=PATH_PTS, device=0):
    """hdsm_local_path_batch: the path step (csrc/path_core.h) for n cases on the device. world int8 [wz][wy][wx] or None (free
    space); off [n][3] local voxel 0 in world voxels, ground_k [n], origin/start/goal [n][3]. Returns paths [n][pmax][3],
    n_path [n], status [n] (0 ok, 1 no free voxel, 2 unreachable, 3 too many points, 4 workspace)."""
    return _local_path("hdsm_local_path_batch", (device,), world, ldim, off, ground_k, origin, start, goal, res, pmax)


def local_path_host(world, ldim, off, ground_k, origin, start, goal, res=0.3, pmax=PATH_PTS):
    """hdsm_local_path_host: the same batch on the CPU (bit for bit what local_path_batch returns)."""
    return _local_path("hdsm_local_path_host", (), world, ldim, off, ground_k, origin, start, goal, res, pmax)


def local_path_dmp_batch(world, ldim, off, ground_k, origin, start, goal, search_rad=1.8, res=0.3, pmax=PATH_PTS, device=0):
    """hdsm_local_path_dmp_batch: local_path_batch in clearance mode (the distance-map planner in a tunnel of radius search_rad round
    the descent, < 0 no tunnel, and ShortenDMPPath). Returns paths, n_path, status, cost [n] (the path's cost, -1 on failure) and
    n_raw [n] (voxels of the planner's chain)."""
    return _local_path("hdsm_local_path_dmp_batch", (device,), world, ldim, off, ground_k, origin, start, goal, res, pmax,
                       search_rad=float(search_rad))


def local_path_dmp_host(world, ldim, off, ground_k, origin, start, goal, search_rad=1.8, res=0.3, pmax=PATH_PTS):
    """hdsm_local_path_dmp_host: the same batch on the CPU (bit for bit what local_path_dmp_batch returns)."""
    return _local_path("hdsm_local_path_dmp_host", (), world, ldim, off, ground_k, origin, start, goal, res, pmax, search_rad=float(search_rad))


LINK_MAX_DELAY = 7  # HDSM_LINK_MAX_DELAY (include/hdsm_swarm.h)


class LinkView:
    """The per-sender link model of the device loop on host arrays (hdsm_link_deliver_host, the source k_deliver runs): the ring of
    the last max_delay + 1 rounds of published records and the view — seen, seen_has, seen_round, shift, counters [n_slots][4] —
    starting, like hdsm_dswarm_set_links, from the records plans0 / has0 held at round -1. deliver(truth) is one link round."""

    def __init__(self, fate, n_slots, n_hor, step_plan, time_aware, plans0, has0):
        self.fate = _i8(fate)
        assert self.fate.ndim == 2
        self.n_rounds, self.n_rob = self.fate.shape
        self.n_slots, self.n_hor, self.step_plan, self.time_aware = int(n_slots), int(n_hor), int(step_plan), 1 if time_aware else 0
        self.max_delay = int(max(0, self.fate.max())) if self.fate.size else 0
        self.ring = np.zeros((self.max_delay + 1, self.n_slots, n_hor + 1, 9))
        self.seen = np.array(plans0, dtype=np.float64, order="C", copy=True).reshape(self.n_slots, n_hor + 1, 9)
        self.seen_has = np.array(has0, dtype=np.uint8, order="C", copy=True).reshape(self.n_slots)
        self.seen_round = np.full(self.n_slots, -1, np.int32)
        self.shift = np.zeros(self.n_slots, np.int32)
        self.counters = np.zeros((self.n_slots, 4), np.int32)
        self.round = 0

    def deliver(self, truth):
        """One link round: truth [n_slots][n_hor+1][9] are the records published in it (raw: a NaN in front = no plan)."""
        truth = _f64(truth).reshape(self.n_slots, self.n_hor + 1, 9)
        call("hdsm_link_deliver_host", self.n_slots, self.n_rob, self.n_hor, self.step_plan, self.n_rounds, self.fate, self.max_delay,
             self.time_aware, self.round, truth, self.ring, self.seen, self.seen_has, self.seen_round, self.shift, self.counters)
        self.round += 1


def _tracks(knots):
    """knots [n_script][n_knots][4] (a single track [n_knots][4] is one agent's) as a contiguous float64 array"""
    knots = _f64(knots)
    if knots.ndim == 2:
        knots = knots[None]
    if knots.ndim != 3 or knots.shape[2] != 4:
        raise HdsmError(HDSM_ERR_BAD_ARG, "tracks [n_script][n_knots][4] of (t, x, y, z) expected")
    return _f64(knots)


def script_records(knots, n_hor, step_plan=1, dt=0.1, predict=0, round=0, device=None):
    """hdsm_script_records_host: the records [n_script][n_hor+1][9] scripted agents on the tracks knots [n_script][n_knots][4] of
    (t, x, y, z) publish in script round `round` (csrc/script_core.h: piecewise linear between the knots, at rest before the first
    and after the last; predict=1: beyond state step_plan the state continues at constant velocity). device given:
    hdsm_script_records_batch, the same through k_script on that device, bit for bit."""
    knots = _tracks(knots)
    records = np.zeros((knots.shape[0], int(n_hor) + 1, 9))
    lead, fn = ((), "hdsm_script_records_host") if device is None else ((int(device),), "hdsm_script_records_batch")
    call(fn, *lead, knots.shape[0], knots.shape[1], knots, int(n_hor), int(step_plan), float(dt), int(predict), int(round), records)
    return records


def track_states(model, ids, planned, T, round=0, device=None):
    """hdsm_track_states_host: (flown [n][9], dist [n]) — the states the agents `ids` (global ids) fly in tracking round `round` in place
    of planned [n][9] = (p, v, a) under the model (params.Tracking, scenarios.gust_model) over the flown interval T = step_plan * dt
    (csrc/track_core.h), and the distance between the two positions. device given: hdsm_track_states_batch, the same through k_track
    on that device, bit for bit."""
    ids, planned = _i32(ids).reshape(-1), _f64(planned)
    if planned.ndim != 2 or planned.shape != (ids.size, 9):
        raise HdsmError(HDSM_ERR_BAD_ARG, "track_states: planned [n][9] for ids [n] expected")
    flown, dist = np.zeros_like(planned), np.zeros(ids.size)
    lead, fn = ((), "hdsm_track_states_host") if device is None else ((int(device),), "hdsm_track_states_batch")
    call(fn, *lead, model, ids.size, ids, planned, float(T), int(round), flown, dist)
    return flown, dist


def command(yaw, n_ref, ref_point, state_before, records, valid, state_after, step_plan=1, dt=0.1, yaw_idx=3, k_p_yaw=1.0, device=None):
    """hdsm_command_host: one round of commands for n agents on plain arrays (csrc/command_core.h) — yaw [n] the yaw before the round,
    n_ref [n] and ref_point [n][3] = traj_ref[yaw_idx][0:3], state_before [n][9] = state_curr before the commit, records [n][n_hor+1][9],
    valid [n] (1 solved, 2 shifted fallback, 0 no plan), state_after [n][9] the state the round ends in. Returns (yaw after the step
    [n], setpoint [n][step_plan] and pose [n] of lib.COMMAND, (steps taken, steps skipped)). device given: hdsm_command_batch, the same
    through k_command on that device, bit for bit."""
    yaw = np.array(yaw, dtype=np.float64, order="C", copy=True).reshape(-1)
    n = yaw.size
    records = _f64(records)
    if records.ndim != 3 or records.shape[0] != n or records.shape[2] != 9:
        raise HdsmError(HDSM_ERR_BAD_ARG, "command: records [n][n_hor+1][9] for yaw [n] expected")
    n_ref, valid = _i32(n_ref).reshape(n), _i32(valid).reshape(n)
    ref_point, state_before, state_after = _f64(ref_point).reshape(n, 3), _f64(state_before).reshape(n, 9), _f64(state_after).reshape(n, 9)
    setpoint, pose, stats = np.zeros((n, int(step_plan)), COMMAND), np.zeros(n, COMMAND), np.zeros(2, np.int64)
    lead, fn = ((), "hdsm_command_host") if device is None else ((int(device),), "hdsm_command_batch")
    call(fn, *lead, n, records.shape[1] - 1, int(step_plan), float(dt), int(yaw_idx), float(k_p_yaw), n_ref, ref_point, state_before, records,
         valid, state_after, yaw, setpoint, pose, stats)
    return yaw, setpoint, pose, (int(stats[0]), int(stats[1]))


def vehicle_default():
    """hdsm_vehicle_default: a Crazyflie-class setting (params.Vehicle), wind and gust 0. Proposals: no flight was measured with them."""
    m = Vehicle()
    call("hdsm_vehicle_default", C.byref(m))
    return m


def vehicle_seat(model, states, yaw):
    """hdsm_vehicle_seat_host: vehicles (lib.VEHICLE_STATE [n]) seated on states [n][9] = (p, v, a) and yaw [n]: at rest in attitude, the
    quaternion of that acceleration and yaw, the thrust that acceleration asks for (clamped)."""
    yaw = _f64(yaw).reshape(-1)
    states = _f64(states).reshape(yaw.size, 9)
    out = np.zeros(yaw.size, VEHICLE_STATE)
    call("hdsm_vehicle_seat_host", model, yaw.size, states, yaw, out)
    return out


def vehicle_fly(model, ids, start, setpoint, planned_end, vstate, step_plan=1, dt=0.1, round=0, device=None):
    """hdsm_vehicle_fly_host: one round of n vehicles (csrc/vehicle_core.h) — ids [n] global ids, start [n][9] knot 0 of the along feed
    (traj_curr[0]), setpoint [n][step_plan] of lib.COMMAND, planned_end [n][9] the state the commit left, vstate [n] of
    lib.VEHICLE_STATE (not modified). Returns (vstate after the round, flown [n][9], dist [n], pose [n] of lib.COMMAND, (agent-rounds
    flown, reseated, sub-steps with the thrust clamped, with a rate clamped)). device given: hdsm_vehicle_fly_batch, the same through
    k_vehicle on that device, bit for bit."""
    ids = _i32(ids).reshape(-1)
    n = ids.size
    start, planned_end = _f64(start).reshape(n, 9), _f64(planned_end).reshape(n, 9)
    setpoint = np.ascontiguousarray(setpoint, dtype=COMMAND).reshape(n, int(step_plan))
    vs = np.array(vstate, dtype=VEHICLE_STATE, order="C", copy=True).reshape(n)
    flown, dist, pose, stats = np.zeros((n, 9)), np.zeros(n), np.zeros(n, COMMAND), np.zeros(4, np.int64)
    lead, fn = ((), "hdsm_vehicle_fly_host") if device is None else ((int(device),), "hdsm_vehicle_fly_batch")
    call(fn, *lead, model, n, ids, int(step_plan), float(dt), int(round), start, setpoint, planned_end, vs, flown, dist, pose, stats)
    return vs, flown, dist, pose, tuple(int(x) for x in stats)


def mission_table(waypoints, count=None):
    """(waypoints float64 [n][n_wp][3], count int32 [n]) as the mission entry points take them; count None: every agent visits all."""
    waypoints = _f64(waypoints)
    if waypoints.ndim != 3 or waypoints.shape[2] != 3:
        raise HdsmError(HDSM_ERR_BAD_ARG, "waypoints [n][n_wp][3] expected")
    count = np.full(waypoints.shape[0], waypoints.shape[1], np.int32) if count is None else _i32(count).reshape(-1)
    if count.size != waypoints.shape[0]:
        raise HdsmError(HDSM_ERR_BAD_ARG, "count [n] for waypoints [n][n_wp][3] expected")
    return waypoints, count


def mission_step(setting, records, states, waypoints, count=None, round=0, goals=None, due=None, device=None):
    """hdsm_mission_step_host: one mission step (csrc/mission_core.h) of n agents in mission round `round` — setting (params.Mission,
    scenarios.mission_setting), records [n] of lib.MISSION_RECORD (not modified), states [n][9], waypoints [n][n_wp][3], count [n]
    (None: all), goals [n][3] and due [n] as they stand (None: zeros). Returns (records after the step, goals, due, summary dict): an
    agent that arrived and is not done has its next waypoint in goals and 1 in due. device given: hdsm_mission_step_batch, the same
    through k_mission on that device, bit for bit."""
    rec = np.array(records, dtype=MISSION_RECORD, order="C", copy=True).reshape(-1)
    n = rec.size
    waypoints, count = mission_table(waypoints, count)
    if waypoints.shape[0] != n or waypoints.shape[1] != setting.n_wp:
        raise HdsmError(HDSM_ERR_BAD_ARG, "mission_step: waypoints [n][setting.n_wp][3] for records [n] expected")
    states = _f64(states).reshape(n, 9)
    goals = np.zeros((n, 3)) if goals is None else np.array(goals, dtype=np.float64, order="C", copy=True).reshape(n, 3)
    due = np.zeros(n, np.uint8) if due is None else np.array(due, dtype=np.uint8, order="C", copy=True).reshape(n)
    summary = MissionSummary()
    lead, fn = ((), "hdsm_mission_step_host") if device is None else ((int(device),), "hdsm_mission_step_batch")
    call(fn, *lead, setting, n, int(round), states, waypoints, count, rec, goals, due, C.byref(summary))
    return rec, goals, due, summary.as_dict()


def assign_groups(groups, n):
    """(n_groups, group_start int32 or None) as the assignment entry points take a partition: None (or fewer than two entries) is one
    group of all n."""
    gs = _i32([] if groups is None else groups).reshape(-1)
    return (0, None) if gs.size < 2 else (gs.size - 1, gs)


def assign(pos, slots, groups=None, active=None, setting=None, device=None):
    """hdsm_assign_host: which agent takes which slot (csrc/assign_core.h) — per neighbour group (groups: group_start [n_groups + 1],
    None one group) the exact minimum of the summed quantised squared distances between the active agents (active [n], None: all) at
    pos [n][3] and the slots [n][3] at the same indices, by the integer auction. setting: params.AssignSetting (None: quantum 0.01 m,
    the default budget). Returns (slot_of int32 [n], -1 for an inactive agent; price int64 [n] by slot, the dual solution; stats, one
    lib.ASSIGN_STATS record per group). device given: hdsm_assign_batch, the same through k_assign on that device, bit for bit."""
    pos, slots = _f64(pos).reshape(-1, 3), _f64(slots).reshape(-1, 3)
    n = pos.shape[0]
    if slots.shape[0] != n:
        raise HdsmError(HDSM_ERR_BAD_ARG, "assign: slots [n][3] for pos [n][3] expected")
    ng, gs = assign_groups(groups, n)
    active = None if active is None else _u8(active).reshape(n)
    slot_of, price, stats = np.full(n, -1, np.int32), np.zeros(n, np.int64), np.zeros(max(ng, 1), ASSIGN_STATS)
    lead, fn = ((), "hdsm_assign_host") if device is None else ((int(device),), "hdsm_assign_batch")
    call(fn, *lead, setting, n, ng, gs, pos, active, slots, slot_of, price, stats)
    return slot_of, price, stats


def command_atan2(y, x):
    """hdsm_command_atan2: the own atan2 of csrc/command_core.h, elementwise."""
    y, x = np.broadcast_arrays(_f64(y), _f64(x))
    y, x = _f64(y).reshape(-1), _f64(x).reshape(-1)
    out = np.zeros(y.size)
    call("hdsm_command_atan2", y.size, y, x, out)
    return out


def command_sincos(x):
    """hdsm_command_sincos: the own (sin, cos) of csrc/command_core.h, elementwise (NaN for |x| >= 2^20)."""
    x = _f64(x).reshape(-1)
    s, c = np.zeros(x.size), np.zeros(x.size)
    call("hdsm_command_sincos", x.size, x, s, c)
    return s, c


def _flight_audit(fn, lead, plans_all, has_plan, step_plan, first, n_local, drone_radius, drone_z_offset, world, worigin, voxel_size):
    plans_all, has_plan = _f64(plans_all), _u8(has_plan)
    n_rob, n_hor = plans_all.shape[0], plans_all.shape[1] - 1
    assert plans_all.ndim == 3 and plans_all.shape[2] == 9 and has_plan.shape == (n_rob,)
    n_local = n_rob - first if n_local is None else int(n_local)
    world, wdim = _world(world)
    worg = None if world is None else _f64(np.asarray(worigin, dtype=np.float64).reshape(3))
    out = np.zeros(max(n_local, 0), AUDIT_ROUND)
    call(fn, *lead, n_rob, plans_all, has_plan, n_hor, int(step_plan), int(first), n_local, drone_radius, drone_z_offset, world, wdim, worg,
         voxel_size, out)
    return out


def flight_audit_host(plans_all, has_plan, step_plan=1, first=0, n_local=None, drone_radius=0.25, drone_z_offset=0.25, world=None,
                      worigin=(0.0, 0.0, 0.0), voxel_size=0.3):
    """hdsm_flight_audit_host: what the agents [first, first + n_local) flew in one round of published records plans_all
    [n_rob][n_hor+1][9] (has_plan [n_rob]): an AUDIT_ROUND record per subject — sep2 (the continuous minimum of the separation
    ratio squared over the step_plan sub-steps and all partners), partner, substep, and the own-track figures on `world`
    (int8 [wz][wy][wx] at voxel_size with voxel (0,0,0) at worigin; None = free space)."""
    return _flight_audit("hdsm_flight_audit_host", (), plans_all, has_plan, step_plan, first, n_local, drone_radius, drone_z_offset, world,
                         worigin, voxel_size)


def flight_audit_batch(plans_all, has_plan, step_plan=1, first=0, n_local=None, drone_radius=0.25, drone_z_offset=0.25, world=None,
                       worigin=(0.0, 0.0, 0.0), voxel_size=0.3, device=0):
    """hdsm_flight_audit_batch: the same audit on the device (k_audit_pack, k_audit, k_audit_track; host arrays in and out), bit
    for bit what flight_audit_host returns."""
    return _flight_audit("hdsm_flight_audit_batch", (device,), plans_all, has_plan, step_plan, first, n_local, drone_radius,
                         drone_z_offset, world, worigin, voxel_size)
