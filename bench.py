#!/usr/bin/env python3
"""bench.py — agent-replans/s of the HIP hot path on BASELINE.json's workload.

One "step" = one replan round of the local shard: ONE launch of the fused kernel (separating planes + exact MIQP for
every local agent) and, for N > 1, ONE RCCL all-gather of the new plans (hdsm_exchange_device, include/hdsm.h).

Workload (config.workload): the configuration BASELINE.json's metric is quoted on — 1024 agents, circular exchange with
R = 1024 / (2 pi) = 163 m (chord 1 m; the shipped 22 m ring would put the agents 0.135 m apart), empty environment,
H = 10, agent_agile_config.yaml weights / limits (BASELINE configs[3]; it fits one GPU). The SAME 1024 agents and the
SAME rounds are used at every N: they are sharded 1024 / N per GPU ("scaling": "strong").

Inputs are produced by SIMULATION, not drawn from a distribution: during the untimed set-up the
swarm is flown in closed loop with the device solver from round 0; the inputs of rounds
[--first-round - warmup, --first-round + steps) are kept resident in HBM and replayed, one recorded round per step. The
TIMED rounds are [--first-round, --first-round + steps) whatever --warmup is; beyond WINDOW_MAX steps the WINDOW_MAX recorded
rounds are replayed cyclically, so that the set-up does not grow with --steps. Default --first-round 165: the rounds in
which the contracting ring reaches the 0.5 m separation limit (from round 167 on, root relaxations turn infeasible by the
hundred: 286 of 1024 instances in round 173; the caller's shift fallback handles them) — the hard part of the flight.

A plain run sets up, warms up, times the --steps steps once and prints the line; the passes that need runs of their own (event
pass, CPU baselines and parity, device-resident loop, secondary workloads, ...) run with --full. --dump-outputs DIR writes what the
last timed step returned.

Prints ONE JSON line (rank 0). `roofline.achieved` = algorithmic bytes per launch (SURVEY.md section 8d formula x agents
per launch) / mean kernel duration measured with HIP events on the launch stream. `roofline.after_prefilter` prices the
same launches by the bytes the kernel really has to touch once the sphere prefilter has discarded distant neighbours
(32-B sphere record per neighbour + 24 B per surviving (neighbour, step) pair, counted by the kernel itself).
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
# Distinct recorded rounds the timed steps replay, cyclically beyond it. Each recorded round costs ~9 ms of set-up flight and ~4 MB of
# inputs (host and HBM) against ~0.1 ms per timed step; 200 rounds cover the squeeze of the default line and stop before the swarm
# gridlocks (by round 1164, half of the instances have no solution and a step takes ~1 ms).
WINDOW_MAX = 200


def algorithmic_bytes(n_rob, N, P, rbar):
    """fp64 bytes one agent-replan must touch."""
    return ((n_rob - 1) * N * 3 * 8 + (N + 1) * 3 * 8 + 9 * 8 + N * 6 * 8 + P * rbar * 4 * 8
            + (N + 1) * 9 * 8 + N * 3 * 8 + P)


def workload_key(scenario, n_rob, N, world, first, K):
    return f"{scenario}_a{n_rob}_h{N}_g{world}_r{first}_k{K}"


def kernel_source_sha16():
    """Identity of the solver kernel's sources: a committed PMC summary is quoted only for the sources it was taken on."""
    h = hashlib.sha256()
    for f in ("hdsm_core.h", "hdsm_wave_gi.h", "hdsm_wave_gib.h", "hdsm_api.hip", "hdsm_types.h"):
        h.update(open(os.path.join(ROOT, "multi_agent_pkgs_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, the command line the
    driver would use) and pass their output through. Rank 0 prints the ONE JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agents", type=int, default=1024, help="total agents of the swarm (the same at every --gpus)")
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--first-round", type=int, default=-1, help="first TIMED closed-loop round (default: 165 for the "
                    "1024-agent circle, 25 otherwise); the warm-up replays the rounds just before it")
    ap.add_argument("--scenario", choices=("circle", "forest", "fwf", "lanes"), default="circle",
                    help="circle: antipodal exchange in an empty world (the bench line). forest: the same circle through the "
                    "pillar forest of env_default_config.yaml scaled to the ring (BASELINE configs[2]). fwf: y-z lattice "
                    "through forest + wall + forest (configs[4]; use --horizon 15). lanes: line formation through a lane "
                    "forest (plumbing check). The last three are single-GPU workloads.")
    ap.add_argument("--radius", type=float, default=0.0, help="circle radius [m], default max(22, agents / 2 pi)")
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="wall-clock budget of the CPU baseline leg")
    ap.add_argument("--repeats", type=int, default=None, help="repetitions of the (warm-up + timed) region; the median is reported "
                    "(default: 1, with --full 3)")
    ap.add_argument("--mip-gap", type=float, default=0.0, help="hdsm_params.mip_gap (0 = exact, the default; the reference runs "
                    "Gurobi at its default MIPGap 1e-4)")
    ap.add_argument("--time-limit-s", type=float, default=0.0, help="hdsm_params.time_limit_s (0 = none; AC:952 sets 0.08)")
    ap.add_argument("--max-nodes", type=int, default=0, help="development: hdsm_params.max_nodes (0 = the default, 2000 branch-and-bound nodes per instance)")
    ap.add_argument("--device-loop-multi", action="store_true", help="(kept for old command lines: the device-resident-loop pass now runs "
                    "with --gpus > 1 by default, last and under a watchdog)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cpu-baseline-corridor", action="store_true", help="skip the orc_safe_corridor comparison of the device-loop pass")
    ap.add_argument("--save-recording", default="", help="development: write the recorded rounds (solver inputs) to this .npz")
    ap.add_argument("--load-recording", default="", help="development: replay the rounds of a --save-recording file instead of flying "
                    "the set-up flight (A/B of execution knobs on IDENTICAL inputs; implies --no-event-pass)")
    ap.add_argument("--cold-start", action="store_true", help="development: hdsm_params.warm_start = 0 (every replan starts from the "
                    "unconstrained optimum; the default line carries the working sets over)")
    ap.add_argument("--no-event-pass", action="store_true", help="skip the HIP-event pass and the host-buffer pass")
    ap.add_argument("--host-reference", action="store_true", help="generate the reference trajectories of the set-up "
                    "flight on the host (csrc/swarm_host.cpp) instead of with the f1 device kernel (hdsm_reference)")
    ap.add_argument("--dist-backend", default="rccl", help="rccl: the product path (hdsm_comm_* / hdsm_exchange_device, "
                    "RCCL linked into libhdsm.so). gloo: testing the multi-rank flow on a box with fewer GPUs than ranks "
                    "(ranks share devices, the all-gather is staged through the host)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short windows of BASELINE configs[2] (forest) and configs[4] (forest + wall "
                    "+ forest, H = 15) that a --full single-GPU circle run appends as secondary_workloads")
    ap.add_argument("--no-weak-record", action="store_true", help="N > 1: skip the secondary weak-scaling record (1024 agents "
                    "per GPU)")
    ap.add_argument("--parity-sample", type=int, default=0, help="after the timed region, replay the timed rounds once more, download the "
                    "device answers and compare this many random instances per round (plus the instances that ended on a budget, up to "
                    "8 per round) with the CPU oracle -> parity_on_timed_rounds (what the secondary workloads of the default line run with; "
                    "a --full circle line compares EVERY timed instance in its cpu_baseline leg instead)")
    ap.add_argument("--parity-seconds", type=float, default=40.0, help="wall-clock budget of the --parity-sample pass (rounds beyond it are skipped)")
    ap.add_argument("--device-loop", action="store_true", help="run the device-resident-loop pass (hdsm_dswarm_round live, with its per-phase "
                    "HIP-event shares and, in obstacle worlds, a bounded orc_safe_corridor comparison) even with --no-event-pass: what the "
                    "forest / fwf secondary records of a --full line carry")
    ap.add_argument("--second-window", type=int, default=-1, help="first round of a second timed window recorded in the same set-up flight "
                    "(default with --full: 100 for the 1024-agent circle line - rounds in which every instance has a solution - else none; 0 = none)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure as well: the event pass (kernel_ms_*, solve "
                    "latency, roofline on the kernel alone), host-buffer and single-instance calls, device-resident loop, CPU baselines with "
                    "their parity check, second window, secondary workloads, three repeats and, N > 1, exchange timing and weak-scaling record. "
                    "Without it a run sets up, warms up, times the --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the last timed step returned "
                    "(traj, ctrl, used, status, obj of every agent) to DIR/<name>.npy as float64")
    args = ap.parse_args()
    if not args.full:   # a plain run: nothing that needs runs of its own besides the timed steps
        args.no_event_pass = args.no_cpu_baseline = args.no_secondary = args.no_weak_record = True
        if args.second_window < 0:
            args.second_window = 0
    if args.repeats is None:
        args.repeats = 3 if args.full else 1
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # (ranks share devices: the gloo flow check of a box with fewer GPUs than ranks; HDSM_BENCH_SAME_DEVICE=1: the test of the
        # line's behaviour when RCCL refuses the communicator — two ranks on one device)
        if args.dist_backend == "gloo" or os.environ.get("HDSM_BENCH_SAME_DEVICE") == "1":
            local_rank = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        # torch.distributed is the LAUNCHER-side plumbing only (rendezvous, broadcast of the RCCL unique id, the barrier
        # and the max-over-ranks of the contract); the data path is hdsm_exchange_device
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)

    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params, agile_ref_config

    N = args.horizon
    prm = agile_params(N, max_rows_static=18, mip_gap=args.mip_gap, time_limit_s=args.time_limit_s, warm_start=not args.cold_start)
    if args.max_nodes > 0:
        prm.max_nodes = args.max_nodes
    P, RS = prm.poly_hor, prm.max_rows_static
    n_rob = args.agents
    radius = args.radius if args.radius > 0 else max(22.0, n_rob / (2 * np.pi))
    first, n_local = swarm.shard_range(n_rob, rank, world)
    per = (n_rob + world - 1) // world
    K, W = args.steps, args.warmup
    R = min(K, WINDOW_MAX)   # distinct recorded rounds; timed step i replays the (i mod R)-th
    first_round = args.first_round if args.first_round >= 0 else (165 if (args.scenario == "circle" and n_rob == 1024 and N == 10) else 25)
    W = min(W, first_round)
    rec_from, rec_to = first_round - W, first_round + R   # recorded rounds [rec_from, rec_to)
    key = workload_key(args.scenario, n_rob, N, world, first_round, K)
    # a second timed window of the same flight (the default line only): rounds before the squeeze, every instance has a solution
    first2 = args.second_window if args.second_window >= 0 else (100 if (args.scenario == "circle" and n_rob == 1024 and N == 10 and first_round == 165) else 0)
    if first2 <= 0 or first2 + R > rec_from or first2 < W or args.load_recording:
        first2 = 0
    rec2_from, rec2_to = first2 - W, first2 + R

    solver = lib.Solver(prm, max(n_local, 1), max(n_rob, world * per), device=dev.index)
    stream = torch.cuda.current_stream()
    comm = None
    exchange_error = None
    if world > 1 and args.dist_backend == "rccl":
        # RCCL prints a version banner on stdout when a communicator is created: keep stdout for the ONE JSON line.
        # hdsm_comm_create (ncclCommInitRank) may FAIL (e.g. ncclInvalidUsage: two ranks on one device) or never come back (a rank
        # that died before the bootstrap): it runs in a thread with a budget, the ranks agree on the outcome through the launcher's
        # gloo group, and without a communicator the line is still produced — host-staged exchange, `exchange_error` says why.
        import threading
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        box = {}
        try:
            uid = [lib.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)

            def make_comm():
                try:
                    box["comm"] = lib.Comm(solver, uid[0], rank, world)
                except BaseException as e:  # noqa: BLE001
                    box["error"] = repr(e)[:300]

            th_c = threading.Thread(target=make_comm, daemon=True)
            th_c.start()
            th_c.join(float(os.environ.get("HDSM_BENCH_COMM_BUDGET_S", "120")))
            if th_c.is_alive():
                box["error"] = "hdsm_comm_create did not return within its budget (HDSM_BENCH_COMM_BUDGET_S)"
        except BaseException as e:  # noqa: BLE001
            box["error"] = repr(e)[:300]
        finally:
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
        errs = [None] * world
        dist.all_gather_object(errs, box.get("error"))
        if any(e is not None for e in errs):
            exchange_error = {"ranks_failed": [k for k, e in enumerate(errs) if e is not None], "first_error": next(e for e in errs if e is not None),
                              "consequence": "no RCCL communicator: the exchange of this line is the host-staged gloo all-gather (flow only); "
                                             "rccl_ranks is null and the weak-scaling record / device loop over RCCL are skipped"}
            if "comm" in box and not th_c.is_alive():
                try:
                    box["comm"].close()
                except Exception:
                    pass
            comm = None
        else:
            comm = box["comm"]
            assert comm.world == world and comm.rank == rank

    # ---------------------------------------------------------------- set-up: closed-loop flight, recording
    def allgather_np(local):  # set-up flight only (host arrays): through the launcher's process group
        t = torch.from_numpy(np.ascontiguousarray(local))
        full = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)
        dist.all_gather_into_tensor(full, t)
        return full.numpy()

    def solve_np(inp, plans, has):
        return solver.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"],
                             inp["A"], inp["b"], plans, has)

    cfg = swarm.default_swarm_config()
    rcfg = agile_ref_config()

    def ref_dev(ids, path, n_path, plans, has, vel_cap=None):  # row f1 on the device: removes the host's O(n_rob^2 N) step
        full, _, pv = solver.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    starts = goals = None
    world_occ = None
    if args.scenario != "circle":
        assert world == 1, "--scenario forest / fwf / lanes are single-GPU workloads"
    if args.scenario == "lanes":
        n_y = min(n_rob, 32)
        assert n_rob % n_y == 0
        starts, goals, world_occ, world_origin = swarm.lane_forest_scenario(n_y, n_rob // n_y, seed=7)
    elif args.scenario == "forest":
        raw, world_origin = sc.forest_for_circle(n_rob, radius=radius, seed=13)
        world_occ = sc.inflate(raw)
    elif args.scenario == "fwf":
        n_y = int(round(np.sqrt(n_rob)))
        assert n_y * n_y == n_rob, "--scenario fwf takes a square number of agents (n x n lattice)"
        starts, goals = sc.lattice_scenario(n_y, n_y)
        raw, world_origin = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
        world_occ = sc.inflate(raw)
        cfg.grid_range[2], cfg.grid_z_min = 12.0, -6.0
    rec_keys = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
    limits_timed = 0   # instances of the timed rounds that ended on a work budget (HDSM_LIMIT), counted in the set-up flight
    if args.load_recording:
        assert world == 1
        args.no_event_pass = True
        z = np.load(args.load_recording)
        rec = [{k: z[k][i] for k in rec_keys} for i in range(z["agent_id"].shape[0])]
        assert len(rec) == rec_to - rec_from, "the recording was made with other --steps / --warmup / --first-round"
        fails, fails_timed, t_setup = int(z["fails"]), int(z["fails_timed"]), 0.0
        rec2, fails2 = [], 0
    else:
        loop = swarm.SwarmLoop(prm, cfg, n_rob, rank=rank, world=world, solve=solve_np,
                               allgather=allgather_np if world > 1 else None, radius=radius,
                               reference=None if args.host_reference else ref_dev, starts=starts, goals=goals)
        if world_occ is not None:
            unrouted = loop.set_world(world_occ, world_origin, route=args.scenario != "lanes")
            assert unrouted == 0
        rec, rec2, fails, fails2, fails_round, limits_round = [], [], 0, 0, [], []
        t_setup = time.perf_counter()
        for r in range(rec_to):
            out = loop.step(record=rec if r >= rec_from else (rec2 if first2 and rec2_from <= r < rec2_to else None))
            if first2 and first2 <= r < rec2_to:
                fails2 += int((out["status"] == 2).sum())
            if r >= rec_from:
                fails += int((out["status"] == 2).sum())
            if r >= first_round:
                fails_round.append(int((out["status"] == 2).sum()))
                limits_round.append(int((out["status"] == 1).sum()))
        t_setup = time.perf_counter() - t_setup
        fails_timed = sum(fails_round[i % R] for i in range(K))
        limits_timed = sum(limits_round[i % R] for i in range(K))
        if args.save_recording:
            np.savez(args.save_recording, fails=fails, fails_timed=fails_timed, **{k: np.stack([x[k] for x in rec]) for k in rec_keys})
    if world > 1:
        cnt = torch.tensor([fails_timed, fails], dtype=torch.int64)
        dist.all_reduce(cnt)
        fails_timed, fails = int(cnt[0]), int(cnt[1])

    def to_device(recs):
        def stack(key_, dtype):
            return torch.from_numpy(np.ascontiguousarray(np.stack([x[key_] for x in recs]), dtype=dtype)).to(dev)
        return (stack("agent_id", np.int32), stack("state", np.float64), stack("ref", np.float64), stack("n_poly", np.int32),
                stack("n_rows", np.int32), stack("A", np.float64), stack("b", np.float64), stack("plans", np.float64),
                stack("has_plan", np.uint8))

    d_win = to_device(rec)
    rows_mean = float(np.mean([x["n_rows"][x["n_rows"] > 0].mean() for x in rec]))
    # outputs: the shard of the NEXT round's plans buffer, gathered into a full buffer when N > 1
    d_traj = torch.zeros((per, N + 1, 9), dtype=torch.float64, device=dev)
    d_ctrl = torch.zeros((per, N, 3), dtype=torch.float64, device=dev)
    d_used = torch.zeros((per, P), dtype=torch.uint8, device=dev)
    d_status = torch.zeros(per, dtype=torch.int32, device=dev)
    d_obj = torch.zeros(per, dtype=torch.float64, device=dev)
    d_next = torch.zeros((world * per, N + 1, 9), dtype=torch.float64, device=dev)
    d_next_has = torch.zeros(world * per, dtype=torch.uint8, device=dev)

    def launch(r, win=None):
        w = d_win if win is None else win
        solver.replan_device(w[0][r], w[1][r], w[2][r], w[3][r], w[4][r], w[5][r], w[6][r], w[7][r], w[8][r],
                             d_traj[:n_local], d_ctrl[:n_local], d_used[:n_local], d_status[:n_local], d_obj[:n_local], stream=stream)

    def exchange():
        if comm is not None:   # ONE collective: plans and has_plan flags travel in the same message
            comm.exchange_device(d_traj, d_next, d_next_has, stream=stream)
        else:                  # gloo: host-staged (flow check only)
            f = torch.empty(d_next.shape, dtype=d_next.dtype)
            dist.all_gather_into_tensor(f, d_traj.cpu())
            d_next.copy_(f)

    def step(r, win=None):
        launch(r, win)
        if world > 1:
            exchange()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_region(win=None):
        """W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides; max over the ranks
        (and this rank's own time)."""
        for r in range(0, W):
            step(r, win)
        barrier()
        t0 = time.perf_counter()
        for i in range(K):
            step(W + i % R, win)
        barrier()
        own = time.perf_counter() - t0
        el = own
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, own

    # ---------------------------------------------------------------- timed region (the contract)
    # W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides, max over the ranks. The
    # region (warm-up included, so every repetition replays the same sequence of warm-start states) is run --repeats times
    # and the line carries the MEDIAN repetition; all of them are listed in "ms_per_step_repeats". One repetition is what the
    # contract describes (a plain run makes one); the others only guard the line against a one-off stall of the box.
    # Before them, the end of the set-up: the recorded window is replayed, untimed, for at least 1000 steps (~0.1 s on the default
    # line), so that the timed steps run on a device in steady state (20 steps last ~2 ms: of three back-to-back repetitions, the
    # first used to run ~3 % slower). The count depends on the arguments only: profiles of separate runs slice the same launches.
    n_pass = -(-1000 // (W + R))
    for _ in range(n_pass):
        for r in range(W + R):
            step(r)
    barrier()
    reps, reps_own = [], []
    for _ in range(max(1, args.repeats)):
        el, own = timed_region()
        reps.append(el), reps_own.append(own)
    elapsed = sorted(reps)[(len(reps) - 1) // 2]
    own_med = sorted(reps_own)[(len(reps_own) - 1) // 2]
    per_rank_ms = [own_med / K * 1e3]
    if world > 1:   # every rank's own time for the K steps (median repetition): where a slow rank sits
        gathered = [None] * world
        dist.all_gather_object(gathered, own_med / K * 1e3)
        per_rank_ms = [float(x) for x in gathered]

    # --dump-outputs: the output buffers of hdsm_replan_device as the LAST timed step left them, every agent of the swarm (the shards
    # of N > 1 gathered in agent order), before any later pass writes into them. The solver stages neighbour rows through atomics, so
    # two runs (and the set-up flights that record their inputs) agree to rounding, not bit for bit.
    dumped = None
    if args.dump_outputs:
        x = rec[W + (K - 1) % R]   # the inputs of that step: a digest tells drifting inputs from drifting outputs
        h = hashlib.sha256()
        for k in rec_keys:
            h.update(np.ascontiguousarray(x[k]).tobytes())
        dig = h.hexdigest()
        if world > 1:
            digs = [None] * world
            dist.all_gather_object(digs, dig)
            dig = hashlib.sha256("".join(digs).encode()).hexdigest()
        dumped = {"round": first_round + (K - 1) % R, "inputs_sha16": dig[:16],
                  "what": "the recorded round the last timed step replayed, whose outputs --dump-outputs wrote, and a digest of its solver "
                          "inputs (agent_id, state, ref, n_poly, n_rows, A, b, plans, has_plan of every rank)"}
        got = {}
        for name, t in (("traj", d_traj), ("ctrl", d_ctrl), ("used", d_used), ("status", d_status), ("obj", d_obj)):
            a = t.double().cpu()
            if world > 1:
                full = torch.empty((world * a.shape[0],) + tuple(a.shape[1:]), dtype=a.dtype)
                dist.all_gather_into_tensor(full, a)
                a = full
            got[name] = a[:n_rob].numpy()
        row_bytes = sum(a[0].size for a in got.values()) * 8 + 8
        keep = (64 << 20) // row_bytes
        if n_rob > keep:   # (a fixed, seeded sample of the agents keeps the files within 64 MB)
            idx = np.sort(np.random.default_rng(0).choice(n_rob, keep, replace=False))
            got = {k: v[idx] for k, v in got.items()}
            got["agent_index"] = idx.astype(np.float64)
        if rank == 0:
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name, a in got.items():
                np.save(os.path.join(args.dump_outputs, name + ".npy"), a)

    # N > 1: the exchange alone (HIP events on the launch stream around hdsm_exchange_device, nothing else queued in between)
    exchange_ms = None
    if world > 1 and args.full:
        n_x = max(K, 20)
        for _ in range(3):
            exchange()
        barrier()
        if comm is not None:
            evx = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_x)]
            for a_, b_ in evx:
                a_.record(stream)
                exchange()
                b_.record(stream)
            barrier()
            xs = np.array([a_.elapsed_time(b_) for a_, b_ in evx])
            how = ("hdsm_exchange_device alone (ONE ncclAllGather of the plan records + the flag kernel), HIP events on the launch "
                   "stream, back to back; p50 / p95 = max over the ranks")
        else:   # host-staged (gloo): wall clock per call, device synchronised on both sides — a flow check, not a figure of the product path
            xs = []
            for _ in range(n_x):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                exchange()
                torch.cuda.synchronize()
                xs.append((time.perf_counter() - t1) * 1e3)
            xs = np.array(xs)
            how = "host-staged gloo all-gather (D2H, all_gather_into_tensor, H2D), wall clock per call: the flow check of a box with fewer GPUs than ranks, NOT the product's exchange"
        t = torch.tensor([float(np.percentile(xs, 50)), float(np.percentile(xs, 95))], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        exchange_ms = {"p50": float(t[0]), "p95": float(t[1]), "this_rank_p50": float(np.percentile(xs, 50)), "samples": len(xs),
                       "bytes_per_rank": per * (N + 1) * 9 * 8, "backend": "rccl" if comm is not None else "gloo-host-staged", "what": how}

    # the second window of the same flight (rounds before the squeeze: every instance has a solution), same timing contract
    second = None
    if first2 and rec2:
        win2 = to_device(rec2)
        reps2 = [timed_region(win2)[0] for _ in range(max(1, args.repeats))]
        el2 = sorted(reps2)[(len(reps2) - 1) // 2]
        second = {"rounds": f"{first2}..{first2 + K - 1}", "warmup_rounds": f"{rec2_from}..{first2 - 1}", "value": n_rob * K / el2,
                  "unit": "agent-replans/s", "ms_per_step": el2 / K * 1e3, "ms_per_step_repeats": [e / K * 1e3 for e in reps2],
                  "failed_instances": fails2, "solved_replans_per_s": (n_rob * K - fails2) / el2,
                  "what": "the same contract (warm-up, K timed steps, barrier + synchronize, max over ranks) on rounds of the same "
                          "flight BEFORE the ring reaches the separation limit: no instance without a solution inflates the count"}
        del win2
        for r in range(0, W):   # (leave the warm-start store as the main window's warm-up leaves it)
            step(r)
        barrier()

    # ---------------------------------------------------------------- second pass: per-launch kernel time (HIP events)
    # Two HIP-event measurements per round, both on the launch stream: around the whole entry point (pre-pass + solver kernel +
    # their launch gaps: the solve latency a caller sees) and, inside the library (hdsm_set_kernel_timing), right before and
    # right after the SOLVER KERNEL alone — the duration the roofline is priced on and the one a rocprofv3 trace shows.
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(R)]
    sph, pairs, it_all, nodes_all, kernel_only_ms = [], [], [], [], []
    dev_out = {}   # device answers of the timed rounds (this replay of the same recorded inputs), kept for the parity check below
    solver.set_kernel_timing(not args.no_event_pass)
    for k, r in enumerate(range(W, W + R) if not args.no_event_pass else []):
        ev[k][0].record(stream)
        launch(r)
        ev[k][1].record(stream)
        kernel_only_ms.append(solver.last_kernel_ms())
        st = solver.last_stats(n_local)
        sw = solver.last_sweep_stats(n_local)
        sph.append(sw["sphere_records"].astype(np.int64).sum()), pairs.append(sw["pairs"].astype(np.int64).sum())
        it_all.append(st["qp_iters"].copy()), nodes_all.append(st["nodes"].copy())
        dev_out[r] = dict(status=d_status[:n_local].cpu().numpy().copy(), traj=d_traj[:n_local].cpu().numpy().copy(),
                          obj=d_obj[:n_local].cpu().numpy().copy(), iters=st["qp_iters"].copy())
    torch.cuda.synchronize()
    solver.set_kernel_timing(False)
    kern_ms = (np.array([a.elapsed_time(b) for a, b in ev]) if not args.no_event_pass
               else np.full(K, elapsed / K * 1e3))
    kernel_only_ms = np.array(kernel_only_ms) if kernel_only_ms else kern_ms
    stats = solver.last_stats(n_local)

    # ---------------------------------------------------------------- third pass: the host-buffer entry point
    # hdsm_replan (host pointers: H2D of the inputs, kernel, D2H of the outputs, synchronous) on the same rounds.
    # Reported next to the line, never as `value`.
    host_ms = host_pinned_ms = None
    if world == 1 and not args.no_event_pass:
        from multi_agent_pkgs_amd.lib import host_register, host_unregister
        keys = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
        out_h = dict(traj=np.zeros((n_local, N + 1, 9)), ctrl=np.zeros((n_local, N, 3)), used=np.zeros((n_local, P), dtype=np.uint8),
                     status=np.zeros(n_local, dtype=np.int32), obj=np.zeros(n_local))

        def host_pass(inputs):
            t1 = time.perf_counter()
            for z in inputs:
                solver.replan(*[z[k] for k in keys], out=out_h, stats=False)
            return (time.perf_counter() - t1) / len(inputs) * 1e3

        # (a) the caller's arrays are ordinary pageable memory (every copy goes through the driver's staging buffer)
        host_ms = host_pass([rec[r] for r in range(W, W + R)])
        # (b) the caller keeps ONE set of arrays, page-locked once with hdsm_host_register, and refills it every round (the
        # refill — the binding writing its inputs — is outside the clock, like the planner code that produces them)
        fixed = {k: np.ascontiguousarray(rec[W][k]).copy() for k in keys}
        for a in list(fixed.values()) + list(out_h.values()):
            host_register(a)
        t_pin = 0.0
        for r in range(W, W + R):
            for k in keys:
                fixed[k][...] = rec[r][k]
            t_pin += host_pass([fixed])
        host_pinned_ms = t_pin / R
        for a in list(fixed.values()) + list(out_h.values()):
            host_unregister(a)

    # ---------------------------------------------------------------- the drop-in's own call shape: ONE instance per call
    # INTEGRATION.md level 2: every Agent process of the reference replaces AC:858-1023 by hdsm_replan with n_inst = 1 against the
    # n_rob plans it has received. A handful of agents, each with its own handle (its own warm-start store, like the GRBModel an
    # Agent keeps), walk the recorded rounds; the timed rounds' calls are clocked one by one on the host (PCIe inclusive).
    single = None
    if world == 1 and not args.no_event_pass and n_local >= 8:
        keys1 = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")
        agents1 = [int(x) for x in np.linspace(0, n_local - 1, 8).astype(int)]
        lat = {"pageable": [], "registered": []}
        status1 = []
        for mode in ("pageable", "registered"):
            for a1 in agents1:
                s1 = lib.Solver(prm, 1, n_rob, device=dev.index)
                o1 = dict(traj=np.zeros((1, N + 1, 9)), ctrl=np.zeros((1, N, 3)), used=np.zeros((1, P), dtype=np.uint8),
                          status=np.zeros(1, dtype=np.int32), obj=np.zeros(1))
                buf = {k: np.ascontiguousarray(rec[0][k][a1:a1 + 1]).copy() for k in keys1}
                buf["plans"], buf["has_plan"] = np.ascontiguousarray(rec[0]["plans"]).copy(), np.ascontiguousarray(rec[0]["has_plan"]).copy()
                pinned = list(buf.values()) + list(o1.values()) if mode == "registered" else []
                for arr in pinned:
                    host_register(arr)
                for r in range(0, W + R):
                    for k in keys1:
                        buf[k][...] = rec[r][k][a1:a1 + 1]
                    buf["plans"][...] = rec[r]["plans"]
                    buf["has_plan"][...] = rec[r]["has_plan"]
                    t1 = time.perf_counter()
                    s1.replan(*[buf[k] for k in keys1], buf["plans"], buf["has_plan"], out=o1, stats=False)
                    dt1 = (time.perf_counter() - t1) * 1e3
                    if r >= W:
                        lat[mode].append(dt1)
                        if mode == "pageable":
                            status1.append(int(o1["status"][0]))
                for arr in pinned:
                    host_unregister(arr)
                s1.close()
        single = {"n_inst": 1, "n_rob": n_rob, "agents": agents1, "calls_per_mode": len(lat["pageable"]),
                  "pageable_ms_p50": float(np.percentile(lat["pageable"], 50)), "pageable_ms_p95": float(np.percentile(lat["pageable"], 95)),
                  "registered_ms_p50": float(np.percentile(lat["registered"], 50)), "registered_ms_p95": float(np.percentile(lat["registered"], 95)),
                  "calls_without_solution": int(sum(1 for x in status1 if x == 2)),
                  "reference_time_limit_ms": 80.0,
                  "what": "hdsm_replan(n_inst = 1) as ONE Agent process of the reference would call it in place of AC:858-1023 (its own handle and "
                          "warm-start store, all n_rob received plans as input), host wall clock per call incl. H2D / kernel / D2H / sync, on the "
                          "timed rounds; registered = the caller's arrays page-locked once (hdsm_host_register). AC:952 gives Gurobi 80 ms"}

    # ---------------------------------------------------------------- fourth pass: the device-resident closed loop, LIVE
    # hdsm_dswarm_round continues the flight where the set-up left it (round first_round + steps): corridor, reference,
    # replan, commit, publish and the all-gather as one chain of launches per round, no host round trip. A secondary record.
    dloop = None
    # (with more than one rank it runs LAST, after the line has been assembled, under a watchdog: the RCCL exchange inside
    # hdsm_dswarm_round had not run on a multi-GPU box when this was written, and a secondary record must not cost the line)
    def device_loop_pass():
        dsw = swarm.DeviceSwarm(loop.shard, solver, world_size=world, device=dev.index)
        dsw.upload_plans(loop.plans_all, loop.has_plan)
        for _ in range(2):
            dsw.round(comm, stream)
        barrier()
        t1 = time.perf_counter()
        for _ in range(K):
            dsw.round(comm, stream)
        barrier()
        dl = time.perf_counter() - t1
        if world > 1:
            t = torch.tensor([dl], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dl = float(t.item())
        _, _, _, failed_d = dsw.download(states=False)
        # where the round goes: a few MORE rounds with HIP events between the launches (hdsm_dswarm_set_phase_timing; never the rounds
        # ms_per_round is taken from: every event record is a barrier packet in front of the next kernel)
        phases = None
        plain = os.environ.get("HDSM_BENCH_DLOOP_PLAIN") == "1"   # (scripts/gpu_dloop_trace.sh: a kernel trace of the live rounds only - no event records, no downloads behind them)
        try:
            if plain:
                raise RuntimeError("skipped: HDSM_BENCH_DLOOP_PLAIN=1")
            dsw.set_phase_timing(True)
            acc, n_t = {}, max(4, min(K, 8))
            for _ in range(n_t):
                dsw.round(comm, stream)
                for k_, v_ in dsw.phase_ms().items():
                    acc[k_] = acc.get(k_, 0.0) + v_ / n_t
            dsw.set_phase_timing(False)
            tot = sum(acc.values())
            phases = {"rounds_timed": n_t, "ms": acc, "share": {k_: (v_ / tot if tot > 0 else 0.0) for k_, v_ in acc.items()}, "ms_sum": tot,
                      "what": "HIP events on the round's stream between the launches of hdsm_dswarm_round, mean over rounds_timed further rounds"}
        except Exception as e:  # noqa: BLE001 (a secondary record)
            phases = {"error": repr(e)[:200]}
        _, _, status_d, failed_d2 = dsw.download(states=False)
        cache = None
        try:
            cache = dsw.cache_stats()
        except Exception as e:  # noqa: BLE001
            cache = {"error": repr(e)[:200]}
        # obstacle worlds, one rank: a bounded comparison of the device corridor (k_corridor) with the literal restatement of
        # GenerateSafeCorridor (oracle/hdsm_oracle.c: orc_safe_corridor, AC:1236-1447) on a sample of agents of two further live rounds
        corridor = None
        if world == 1 and world_occ is not None and rank == 0 and not args.no_cpu_baseline_corridor and not plain:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import corridor_oracle as co
                from oracle import pyoracle as orc_c
                rng_c = np.random.default_rng(5)
                n_chk = n_same = n_stop = 0
                t_c = time.perf_counter()
                for _ in range(2):
                    dsw.download(states=True)
                    pre, prm_s, cfg_s, w_s, wo_s = co.export_agents(loop.shard)
                    dsw.round(comm, stream)
                    dsw.download(states=True)
                    post = co.export_agents(loop.shard)[0]
                    for a_ in rng_c.choice(n_local, min(24, n_local), replace=False):
                        rc_o, want = co.oracle_corridor(orc_c.lib(), prm_s, cfg_s, w_s, wo_s, pre[int(a_)])
                        n_chk += 1
                        if rc_o != 0 or post[int(a_)].corridor_rc != 0:
                            n_stop += 1
                            n_same += int(rc_o != 0 and post[int(a_)].corridor_rc != 0)
                        else:
                            n_same += int(co.same_corridor(co.product_corridor(post[int(a_)]), want))
                corridor = {"agents_compared": n_chk, "identical_bit_for_bit": n_same, "stopped_in_both": n_stop, "seconds": time.perf_counter() - t_c,
                            "what": "k_corridor of two further live rounds against orc_safe_corridor (oracle/hdsm_oracle.c, the literal restatement of "
                                    "AC:1236-1447) on the same pre-round agent states: polyhedra, rows and seeds bit for bit"}
            except Exception as e:  # noqa: BLE001
                corridor = {"error": repr(e)[:300]}
        prof = None
        if os.environ.get("HDSM_LIBRARY"):  # a -DCD_PROFILE development build: where the corridor kernel's cycles go
            import ctypes
            L = lib.load()
            if hasattr(L, "hdsm_swarm_corridor_profile"):
                cnt = (ctypes.c_ulonglong * 16)()
                L.hdsm_swarm_corridor_profile(cnt)
                names = ["seed search", "plane rows", "move loop", "rim / far write-out", "allowance", "edge state machine", "shape-aware side tests",
                         "trial layers", "accept (copy, append, mark)", "rows", "world maps", "layer (0..3 inside)", "corridor step", "decompositions in it"]
                ar = max(1, int(cnt[14]))
                prof = {"agent_rounds": int(cnt[14]), "decompositions": int(cnt[15]), "cycles_per_agent_round": {names[i]: int(cnt[i]) / ar for i in range(14)}}
        res = {"rounds": f"{rec_to + 2}..{rec_to + 1 + K}", "ms_per_round": dl / K * 1e3, "agent_replans_per_s": n_rob * K / dl,
               "instances_without_solution_this_rank": int(failed_d), "instances_without_solution_last_round": int((status_d == 2).sum()),
               "instances_on_a_budget_last_round": int((status_d == 1).sum()), "ranks": world,
               "phases": phases, "polyhedron_cache": cache, "corridor_parity": corridor,
               "what": "hdsm_dswarm_round live: corridor (f2) -> reference (f1) -> replan -> commit -> publish -> exchange, one stream"}
        if prof:
            res["corridor_profile"] = prof
        dsw.close()
        return res

    if (not args.no_event_pass or args.device_loop) and world == 1 and not args.load_recording:
        try:
            dloop = device_loop_pass()
        except Exception as e:  # noqa: BLE001 (a secondary record must not cost the line)
            dloop = {"error": repr(e)[:300]}

    # ---------------------------------------------------------------- N > 1: secondary WEAK-scaling record
    # The line above shards the SAME 1024 agents over the ranks (strong scaling: a round cannot end before its slowest instance,
    # so it says little about the exchange). This record fixes the work PER GPU instead: 1024 agents per GPU on a ring of
    # 1024 N agents (R = n / 2 pi, the same 1 m chord), every rank solving its 1024 instances against all 1024 N published plans,
    # one RCCL all-gather of the new plans per round. Early rounds of the flight (the squeeze of a ring that large is thousands of
    # rounds away); same timing contract.
    weak = None
    if world > 1 and args.scenario == "circle" and not args.no_weak_record:
        per_w = int(os.environ.get("HDSM_BENCH_WEAK_PER_GPU", "1024"))
        n_w = per_w * world
        first_w = 25
        solver_w = lib.Solver(prm, per_w, n_w, device=dev.index)

        def solve_w(inp, plans, has):
            return solver_w.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

        def ref_w(ids, path, n_path, plans, has, vel_cap=None):
            full, _, pv = solver_w.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
            return full, pv

        loop_w = swarm.SwarmLoop(prm, cfg, n_w, rank=rank, world=world, solve=solve_w, allgather=allgather_np,
                                 radius=n_w / (2 * np.pi), reference=ref_w)
        rec_w = []
        for r in range(first_w + R):
            loop_w.step(record=rec_w if r >= first_w - W else None)

        def stack_w(key_, dtype):
            return torch.from_numpy(np.ascontiguousarray(np.stack([x[key_] for x in rec_w]), dtype=dtype)).to(dev)

        w_agent, w_state, w_ref = stack_w("agent_id", np.int32), stack_w("state", np.float64), stack_w("ref", np.float64)
        w_npoly, w_nrows = stack_w("n_poly", np.int32), stack_w("n_rows", np.int32)
        w_A, w_b = stack_w("A", np.float64), stack_w("b", np.float64)
        w_plans, w_has = stack_w("plans", np.float64), stack_w("has_plan", np.uint8)
        w_traj = torch.zeros((per_w, N + 1, 9), dtype=torch.float64, device=dev)
        w_ctrl = torch.zeros((per_w, N, 3), dtype=torch.float64, device=dev)
        w_used = torch.zeros((per_w, P), dtype=torch.uint8, device=dev)
        w_status = torch.zeros(per_w, dtype=torch.int32, device=dev)
        w_obj = torch.zeros(per_w, dtype=torch.float64, device=dev)
        w_next = torch.zeros((n_w, N + 1, 9), dtype=torch.float64, device=dev)
        w_next_has = torch.zeros(n_w, dtype=torch.uint8, device=dev)

        def step_w(r):
            solver_w.replan_device(w_agent[r], w_state[r], w_ref[r], w_npoly[r], w_nrows[r], w_A[r], w_b[r], w_plans[r], w_has[r],
                                   w_traj, w_ctrl, w_used, w_status, w_obj, stream=stream)
            if comm is not None:
                comm.exchange_device(w_traj, w_next, w_next_has, stream=stream)
            else:   # gloo: host-staged (flow check only)
                f_w = torch.empty(w_next.shape, dtype=w_next.dtype)
                dist.all_gather_into_tensor(f_w, w_traj.cpu())
                w_next.copy_(f_w)

        reps_w = []
        for _ in range(max(1, args.repeats)):
            for r in range(0, W):
                step_w(r)
            barrier()
            t0 = time.perf_counter()
            for i in range(K):
                step_w(W + i % R)
            barrier()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            reps_w.append(float(t.item()))
        el_w = sorted(reps_w)[(len(reps_w) - 1) // 2]
        weak = {"scaling": "weak", "agents": n_w, "agents_per_gpu": per_w, "n_gpus": world, "value": n_w * K / el_w,
                "unit": "agent-replans/s", "ms_per_step": el_w / K * 1e3, "ms_per_step_repeats": [e / K * 1e3 for e in reps_w],
                "steps": K, "warmup": W, "rounds": f"{first_w}..{first_w + R - 1}",
                "exchange_bytes_per_rank_per_round": per_w * (N + 1) * 9 * 8,
                "exchange": "RCCL all-gather (hdsm_exchange_device)" if comm is not None else "host-staged gloo all-gather (flow check only)",
                "what": f"{per_w} agents per GPU on a ring of {n_w} (R = n / 2 pi): every rank solves its {per_w} instances against "
                        f"all {n_w} plans + ONE RCCL all-gather per round; same barrier / max-over-ranks contract as the line"}
        solver_w.close()

    # ---------------------------------------------------------------- CPU baseline (rank 0, N = 1 only)
    cpu = None
    parity = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # CPU restatement (oracle/hdsm_oracle.c) on a BOUNDED SAMPLE of the same timed rounds, farmed over all host
        # cores: one task = a block of 16 agents of one recorded round solved one after the other by one thread (the
        # reference's one-process-per-agent, Threads=1 deployment); as many tasks as fit the budget.
        from concurrent.futures import ThreadPoolExecutor
        from oracle import pyoracle as orc
        orc.lib()
        cores = os.cpu_count() or 1
        BLK = 16
        blocks = [(r, a) for r in range(W, W + R) for a in range(0, n_local, BLK)]
        rng = np.random.default_rng(0)
        rng.shuffle(blocks)

        ora_out = {}   # oracle answers per block: what the device answers of the SAME recorded rounds are compared with

        def one(ra):
            r, a = ra
            x = rec[r]
            sl = slice(a, min(a + BLK, n_local))
            o = orc.replan(prm, x["agent_id"][sl], x["state"][sl], x["ref"][sl], x["n_poly"][sl], x["n_rows"][sl], x["A"][sl],
                           x["b"][sl], x["plans"], x["has_plan"], n_threads=1)
            ora_out[(r, a)] = (o["status"], o["traj"], o["obj"])
            return sl.stop - sl.start

        # first batch: one block per thread, timed in parallel (the oracle's plane sweeps are memory-heavy: throughput with
        # all cores busy is not cores x the single-thread rate); then as many more batches as fit the budget
        t1 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=cores) as ex:
            done = sum(ex.map(one, [blocks[i % len(blocks)] for i in range(cores)]))
            dt_first = time.perf_counter() - t1
            extra = int(max(0, min((args.cpu_seconds - dt_first) / max(dt_first, 1e-3), 40))) * cores
            if extra:
                done += sum(ex.map(one, [blocks[(cores + i) % len(blocks)] for i in range(extra)]))
        n_tasks = cores + extra
        tasks = range(n_tasks)
        dt_cpu = time.perf_counter() - t1
        cpu = {"value": done / dt_cpu, "unit": "agent-replans/s", "cores": cores, "kind": "port",
               "sample": f"{n_tasks} blocks of {BLK} agents drawn from the {R} timed rounds ({done} agent-replans) on the CPU "
                         f"restatement (oracle/hdsm_oracle.c: cold-started dense active set, not Gurobi), one block per "
                         f"thread, {cores} threads",
               "seconds": dt_cpu, "per_core_replans_per_s": done / dt_cpu / min(cores, len(tasks))}
        # The bench verifies what it times: the device answers of the timed rounds (downloaded in the event pass: the same
        # recorded inputs through the same kernel) against the oracle answers the baseline leg has just computed, block by block.
        if dev_out:
            n_cmp = n_mis = n_fail = n_fail0 = n_nov = 0
            d_traj_max = d_obj_max = 0.0
            for (r, a), (o_st, o_traj, o_obj) in ora_out.items():
                g = dev_out[r]
                sl = slice(a, a + len(o_st))
                g_st = g["status"][sl]
                verdict = o_st != 1   # (an oracle answer that ended on its own budget is no verdict)
                n_nov += int((~verdict).sum())
                n_cmp += int(verdict.sum())
                n_mis += int((g_st[verdict] != o_st[verdict]).sum())
                both = verdict & (o_st == 0) & (g_st == 0)
                if both.any():
                    d_traj_max = max(d_traj_max, float(np.abs(g["traj"][sl][both] - o_traj[both]).max()))
                    d_obj_max = max(d_obj_max, float((np.abs(g["obj"][sl][both] - o_obj[both]) / np.maximum(1.0, np.abs(o_obj[both]))).max()))
                nos = verdict & (o_st == 2)
                n_fail += int(nos.sum())
                n_fail0 += int((nos & (g["iters"][sl] == 0)).sum())
            parity = {"instances_compared": n_cmp, "status_mismatches": n_mis, "max_abs_traj_diff": d_traj_max,
                      "max_rel_obj_diff": d_obj_max, "no_solution_compared": n_fail, "no_solution_first_sweep_exits_compared": n_fail0,
                      "oracle_without_verdict": n_nov, "instances_in_timed_rounds": R * n_local,
                      "what": "device answers (status, trajectory, objective) of the timed rounds, downloaded in the event pass, against "
                              "the CPU oracle on the same recorded inputs (every 16-agent block the baseline leg solved); "
                              "first-sweep exits = instances the kernel ended as infeasible without an active-set operation"}

    # ---------------------------------------------------------------- bounded parity pass (--parity-sample; the secondary workloads)
    # The timed rounds once more (same warm-up, same order: the warm-start states of the timed repetitions), the device answers
    # downloaded round by round and a bounded sample compared with the CPU oracle: M random instances per round + the instances that
    # ended on a work budget (up to 8 per round; their incumbent must not beat the proven optimum). H <= 10: the oracle's step-ordered
    # search first, its second order (most infeasible step first) where that runs into its budget; H > 10: the second order. An
    # oracle answer that ended on ITS budget is no verdict.
    if rank == 0 and world == 1 and args.parity_sample > 0 and parity is None:
        from oracle import pyoracle as orc
        orc.lib()
        cores = os.cpu_count() or 1
        rng_p = np.random.default_rng(11)
        keys_p = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b")
        for r in range(0, W):
            launch(r)
        outs = {}
        for r in range(W, W + R):
            launch(r)
            torch.cuda.synchronize()
            outs[r] = dict(status=d_status[:n_local].cpu().numpy().copy(), traj=d_traj[:n_local].cpu().numpy().copy(),
                           obj=d_obj[:n_local].cpu().numpy().copy(), flags=solver.last_sweep_stats(n_local)["flags"].copy())

        def proved(x, sub, hint=None):
            if N <= 10:
                bounded = prm.copy()
                bounded.max_nodes, bounded.max_qp_iters = 100000, 1000000
                o = orc.replan(bounded, *[x[k][sub] for k in keys_p], x["plans"], x["has_plan"], n_threads=cores)
                again = np.where(o["status"] == 1)[0]
            else:
                o, again = None, np.arange(len(sub))
            if len(again):
                big = prm.copy()
                big.max_nodes, big.max_qp_iters = 200000, 30000000
                o2 = orc.replan(big, *[x[k][sub[again]] for k in keys_p], x["plans"], x["has_plan"], n_threads=cores, search=1,
                                obj_hint=None if hint is None else hint[again])
                if o is None:
                    return o2
                for k in ("traj", "status", "obj"):
                    o[k][again] = o2[k]
            return o

        # Two legs. (1) EVERY answer the device returned without a proof — the instances that ended on a work budget (their incumbent must
        # not beat, and is expected to equal, the oracle's PROVEN optimum) and the instances it called infeasible (the oracle must prove
        # that too) — of every timed round, as far as --parity-seconds goes (2/3 of the budget at most); checked / total are in the record.
        # (2) a random sample of the proven answers per round with what is left.
        t_par = time.perf_counter()
        n_cmp = n_mis = n_nov = n_lim = n_lim_proved = n_lim_beaten = n_lim_above = rounds_done = 0
        n_nos = n_nos_agree = n_nos_mis = n_nos_nov = unproven_rounds = 0
        d_traj_max = d_obj_max = lim_gap_max = 0.0
        lim_total = int(sum((outs[r]["status"] == 1).sum() for r in outs))
        nos_total = int(sum((outs[r]["status"] == 2).sum() for r in outs))
        for r in range(W, W + R):   # leg 1
            if time.perf_counter() - t_par > args.parity_seconds * 2.0 / 3.0:
                break
            x, g = rec[r], outs[r]
            lim = np.where(g["status"] == 1)[0]
            if len(lim):   # incumbents without a proof: hinted search for the optimum (the hint only prunes)
                ol = proved(x, lim, hint=g["obj"][lim] * (1 + 1e-9))
                n_lim += len(lim)
                for t_, a_ in enumerate(lim):
                    if ol["status"][t_] == 0:
                        n_lim_proved += 1
                        gap = float((g["obj"][a_] - ol["obj"][t_]) / max(1.0, abs(ol["obj"][t_])))
                        lim_gap_max = max(lim_gap_max, gap)
                        n_lim_beaten += int(gap < -1e-7)
                        n_lim_above += int(gap > 1e-7)
            nos = np.where(g["status"] == 2)[0]
            if len(nos):
                on = proved(x, nos)
                n_nos += len(nos)
                n_nos_agree += int((on["status"] == 2).sum())
                n_nos_mis += int((on["status"] == 0).sum())
                n_nos_nov += int((on["status"] == 1).sum())
            unproven_rounds += 1
        for r in range(W, W + R):   # leg 2
            if time.perf_counter() - t_par > args.parity_seconds:
                break
            x, g = rec[r], outs[r]
            cand = np.where(g["status"] == 0)[0]
            if len(cand) == 0:
                rounds_done += 1
                continue
            sub = np.sort(rng_p.choice(cand, min(args.parity_sample, len(cand)), replace=False))
            o = proved(x, sub)
            verdict = o["status"] != 1
            n_nov += int((~verdict).sum())
            n_cmp += int(verdict.sum())
            n_mis += int((g["status"][sub][verdict] != o["status"][verdict]).sum())
            both = verdict & (o["status"] == 0) & (g["status"][sub] == 0)
            if both.any():
                d_traj_max = max(d_traj_max, float(np.abs(g["traj"][sub][both] - o["traj"][both]).max()))
                d_obj_max = max(d_obj_max, float((np.abs(g["obj"][sub][both] - o["obj"][both]) / np.maximum(1.0, np.abs(o["obj"][both]))).max()))
            rounds_done += 1
        parity = {"instances_compared": n_cmp + n_nos - n_nos_nov, "status_mismatches": n_mis + n_nos_mis, "max_abs_traj_diff": d_traj_max, "max_rel_obj_diff": d_obj_max,
                  "oracle_without_verdict": n_nov + n_nos_nov, "rounds_checked": rounds_done, "sample_per_round": args.parity_sample,
                  "limit_instances_checked": n_lim, "limit_instances_in_replay": lim_total,
                  "limit_incumbents_with_proven_optimum": n_lim_proved,
                  "limit_incumbent_below_optimum": n_lim_beaten, "limit_incumbent_above_optimum": n_lim_above, "limit_incumbent_max_rel_gap": lim_gap_max,
                  "no_solution_checked": n_nos, "no_solution_in_replay": nos_total, "no_solution_oracle_agrees": n_nos_agree,
                  "no_solution_oracle_finds_a_solution": n_nos_mis, "no_solution_oracle_without_verdict": n_nos_nov,
                  "rounds_checked_for_unproven_answers": unproven_rounds,
                  "failed_instances_in_replay": nos_total,
                  "instances_in_timed_rounds": R * n_local, "seconds": time.perf_counter() - t_par,
                  "what": "a replay of the timed rounds after the timed region (same recorded inputs, same warm-up). Leg 1: EVERY instance the device "
                          "ended on a budget (its incumbent against the oracle's PROVEN optimum: below = a wrong answer, above = a valid but "
                          "suboptimal incumbent, as AC:948-952 lets Gurobi return at its time limit) and EVERY instance it called infeasible (the oracle "
                          "must prove that), round by round within 2/3 of --parity-seconds; leg 2: a random sample of the proven answers per round "
                          "(status, trajectory, objective) against the oracle with a PROOF (second search order where the step-ordered one runs "
                          "into its budget; an oracle answer without proof is no verdict)"}

    # ---------------------------------------------------------------- secondary workloads (default single-GPU line only)
    # BASELINE configs[2] and configs[4] as short windows, each a run of this script in its own process (own handle, own set-up
    # flight); reported next to the line, never as `value`.
    secondary = None
    if rank == 0 and world == 1 and args.scenario == "circle" and not args.no_secondary and not args.load_recording and not args.no_event_pass:
        import subprocess
        secondary = []
        cfg3 = ["--scenario", "forest", "--agents", "256", "--horizon", "10", "--first-round", "60", "--steps", "8", "--warmup", "2"]
        cfg5 = ["--scenario", "fwf", "--agents", "4096", "--horizon", "15", "--first-round", "8", "--steps", "6", "--warmup", "2"]
        # (the third record: cfg 5 at Gurobi's default MIPGap, 1e-4 — the optimality tolerance the reference itself runs with; the
        # line's own --mip-gap, 0 = proven optimal unless a limit is hit, applies to the first two)
        for extra, gap in ((cfg3, args.mip_gap), (cfg5, args.mip_gap), (cfg5, 1e-4)):
            if gap == 1e-4 and args.mip_gap == 1e-4:
                continue
            cmd = [sys.executable, os.path.abspath(__file__)] + extra + ["--no-cpu-baseline", "--no-secondary", "--no-event-pass", "--repeats", "3",
                                                                        "--mip-gap", str(gap), "--time-limit-s", str(args.time_limit_s),
                                                                        "--parity-sample", "128" if gap == 0.0 else "0",
                                                                        "--parity-seconds", "75" if extra is cfg5 else "60"]
            if gap == args.mip_gap:   # (the record at Gurobi's MIPGap repeats the window only: no second device-loop pass)
                cmd.append("--device-loop")
            # (a profiler attached to this process must see this line's launches only: the children run without its preload)
            child_env = {k: v for k, v in os.environ.items() if not k.startswith(("ROCPROF", "ROCP_", "ROCTRACER", "ROCTX"))}
            pre = [x for x in child_env.pop("LD_PRELOAD", "").split(":") if x and "rocprof" not in x and "roctracer" not in x]
            if pre:
                child_env["LD_PRELOAD"] = ":".join(pre)
            try:
                t1 = time.perf_counter()
                pr = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=child_env)
                z = json.loads(pr.stdout.strip().splitlines()[-1])
                secondary.append({"workload_key": z["config"]["workload_key"], "workload": z["config"]["workload"], "mip_gap": gap, "value": z["value"], "unit": z["unit"],
                                  "ms_per_step": z["ms_per_step"], "ms_per_step_repeats": z["ms_per_step_repeats"],
                                  "roofline_frac": z["roofline"]["frac"], "limit_instances": z["limit_instances_timed_rounds"],
                                  "failed_instances": z["failed_instances_timed_rounds"], "nodes_max": z["solver_stats_timed_rounds"]["nodes_max"],
                                  "parity_on_timed_rounds": z.get("parity_on_timed_rounds"),
                                  "device_resident_loop": z.get("device_resident_loop"),
                                  "wall_s": time.perf_counter() - t1,
                                  "what": "ms_per_step = wall clock per replayed round (pre-pass + kernels, inputs resident in HBM); roofline_frac "
                                          "is priced on it (no separate event pass)"})
            except Exception as e:  # a secondary record must not put the line at risk
                secondary.append({"args": extra, "error": repr(e)[:300]})

    # ---------------------------------------------------------------- the honest CPU neighbour (rank 0, N = 1 only)
    # oracle/hdsm_cpu_port.c: the PRODUCT's algorithm (lazy closed-form planes behind the sphere prefilter, normalised pick rule, warm
    # start from the agent's previous replan) as plain C, one host thread per block of agents walking the recorded rounds in order;
    # the warm-up rounds build the warm-start stores, the timed rounds are the ones the GPU line times. Bench-only code.
    cpu_warm = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.scenario == "circle":
        from oracle import pycpuport as port
        cores = os.cpu_count() or 1
        reps_w, last = [], None
        t1 = time.perf_counter()
        while not reps_w or (time.perf_counter() - t1 < min(args.cpu_seconds, 6.0) and len(reps_w) < 9):
            last, secs = port.replay(prm, rec, W, cores)
            reps_w.append(secs)
        secs = sorted(reps_w)[(len(reps_w) - 1) // 2]
        n_cmp = n_mis = 0
        d_max = 0.0
        for r in range(W, W + R):   # its answers against the device's, every instance of the timed rounds
            if r not in dev_out:
                continue
            g = dev_out[r]
            st_c = last["status"][r]
            n_cmp += len(st_c)
            n_mis += int((st_c != g["status"]).sum())
            both = (st_c == 0) & (g["status"] == 0)
            if both.any():
                d_max = max(d_max, float(np.abs(last["traj"][r][both] - g["traj"][both]).max()))
        cpu_warm = {"value": R * n_local / secs, "unit": "agent-replans/s", "cores": cores, "kind": "port-warm",
                    "sample": f"all {R * n_local} agent-replans of the {R} timed rounds, {cores} threads, each owning a block of agents and walking "
                              f"the rounds in order (warm-up rounds {rec_from}..{first_round - 1} build the warm-start stores, untimed); "
                              "oracle/hdsm_cpu_port.c = the kernel's algorithm (lazy closed-form planes, sphere prefilter, normalised pick rule, "
                              "warm start) as scalar C with a textbook dense factorisation — not Gurobi, not a tuned CPU solver",
                    "seconds": secs, "seconds_repeats": reps_w, "per_core_replans_per_s": R * n_local / secs / cores,
                    "active_set_operations_mean": float(last["qp_iters"][W:].mean()), "branch_and_bound_fallbacks": int(last["fallbacks"]),
                    "vs_device": {"instances_compared": n_cmp, "status_mismatches": n_mis, "max_abs_traj_diff": d_max}}

    if rank == 0:
        value = n_rob * K / elapsed
        B = algorithmic_bytes(n_rob, N, P, rows_mean)
        mean_ms = float(kernel_only_ms.mean())   # the solver kernel alone (see the event pass)
        achieved = B * n_local / (mean_ms * 1e-3) / 1e9
        after = None
        if sph:
            fixed = B - (n_rob - 1) * N * 24   # everything but the neighbour positions
            need = (np.array(sph) * 32 + np.array(pairs) * 24 + fixed * n_local).mean()
            a2 = need / (mean_ms * 1e-3) / 1e9
            after = {"bytes_per_launch": float(need), "achieved": a2, "frac": a2 / HBM_PEAK_GBS,
                     "what": "32 B per sphere record read + 24 B per (neighbour, step) pair that survived the prefilter, "
                             "counted by the kernel over all sweeps, + the per-instance inputs / outputs"}
        traffic, traffic_src = None, None
        src_sha = kernel_source_sha16()
        pmc = os.path.join(ROOT, "profiles", f"pmc_{key}.json")
        if os.path.exists(pmc):   # only a PMC summary taken on THIS workload (same agents, rounds, GPUs) AND on these kernel
            try:                  # sources is quoted: after a kernel change the figure is null until the counters are re-collected
                z = json.load(open(pmc))
                if z.get("workload_key") == key and z.get("kernel_source_sha16") == src_sha:
                    traffic, traffic_src = z.get("hbm_bytes_per_launch"), os.path.relpath(pmc, ROOT)
            except Exception:
                traffic = None
        names = {"circle": f"{n_rob} agents circular exchange (R = {radius:g} m), empty env",
                 "forest": f"{n_rob} agents circular exchange (R = {radius:g} m) through a pillar forest (0.2 pillars / m^2, "
                           f"corridors by voxel decomposition, <= {int(max(x['n_rows'].max() for x in rec))} static rows)",
                 "fwf": f"{n_rob} agents on a y-z lattice through forest + wall + forest (corridors by voxel decomposition)",
                 "lanes": f"{n_rob} agents in line formation through a lane forest"}
        it_cat = np.concatenate(it_all) if it_all else stats["qp_iters"]
        line = {
            "metric": "agent QP-replans/sec", "value": value, "unit": "agent-replans/s", "n_gpus": world,
            "steps": K, "warmup": W, "ms_per_step": elapsed / K * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": names[args.scenario] + f", H={N}, poly_hor={P}, closed-loop rounds "
                                   f"{first_round}..{first_round + R - 1} replayed" + (f" cyclically over {K} steps" if K > R else "")
                                   + f" (warm-up: rounds {rec_from}..{first_round - 1})",
                       "workload_key": key, "mip_gap": args.mip_gap, "time_limit_s": args.time_limit_s, "agents": n_rob, "agents_per_gpu": n_local, "horizon": N, "poly_hor": P,
                       "parallelism": f"agents sharded over {world} GPU(s), one RCCL all-gather per round"
                                      if world > 1 else "one GPU"},
            "p50_solve_latency_ms": float(np.percentile(kern_ms, 50)),
            "p95_solve_latency_ms": float(np.percentile(kern_ms, 95)),
            "kernel_ms_mean": mean_ms, "kernel_ms_p50": float(np.percentile(kernel_only_ms, 50)),
            "kernel_ms_p95": float(np.percentile(kernel_only_ms, 95)), "entry_point_ms_mean": float(kern_ms.mean()),
            "kernel_ms_what": ("kernel_ms_* = k_replan alone (HIP events inside the library, after the pre-pass) — what the "
                               "roofline is priced on and what a rocprofv3 trace shows; p50/p95_solve_latency_ms and "
                               "entry_point_ms_mean = the whole hdsm_replan_device call on an idle stream (pre-pass, kernel, launch gaps)")
                              if not args.no_event_pass else
                              "no event pass in this run (--full runs one): kernel_ms_*, p50/p95_solve_latency_ms, entry_point_ms_mean "
                              "and the roofline are priced on ms_per_step",
            "host_buffer_path": None if host_ms is None else {
                "ms_per_round": host_ms, "agent_replans_per_s": n_rob / (host_ms * 1e-3),
                "ms_per_round_registered_arrays": host_pinned_ms,
                "what": "hdsm_replan with host pointers (PCIe-inclusive: H2D inputs, kernel, D2H outputs, sync), output arrays allocated once; "
                        "registered = the caller's arrays page-locked once with hdsm_host_register (DMA without staging, results "
                        "delivered into them by the device)"},
            "device_resident_loop": dloop,
            "rccl_ranks": comm.world if comm is not None else (1 if world == 1 else None),
            "exchange": ("none (one rank)" if world == 1 else ("RCCL all-gather (hdsm_exchange_device)" if comm is not None
                                                               else "host-staged gloo all-gather (flow check only)")),
            "exchange_error": exchange_error,
            "weak_scaling_record": weak,
            "weak_scaling_value": None if weak is None else weak["value"],
            "scaling_note": None if world == 1 else (
                "`value` is STRONG scaling of one 1024-agent swarm (BASELINE configs[3]): a round cannot end before its slowest instance, "
                "about 75 us on whichever GPU it lives, so the curve is flat by construction (sharding this swarm buys nothing but "
                "the exchange cost). What the exchange costs at constant work per GPU is in weak_scaling_record / weak_scaling_value "
                "(1024 agents per GPU, ring of 1024 N agents, one RCCL all-gather per round, same timing contract)"),
            "failed_instances_timed_rounds": fails_timed, "failed_instances_recorded": fails, "limit_instances_timed_rounds": limits_timed,
            "setup_flight_s": t_setup,
            "dumped_step": dumped,
            "ms_per_step_repeats": [e / K * 1e3 for e in reps],
            "k_replan_launch_sequence": {"setup_flight": rec_to, "untimed_pass": n_pass * (W + R), "warmup": W, "timed": K,
                                         "repeats_of_warmup_plus_timed": len(reps), "event_pass": 0 if args.no_event_pass else R,
                                         "host_pass": R if host_ms is not None else 0},
            "solver_stats_timed_rounds": {"qp_iters_max": int(it_cat.max()), "qp_iters_mean": float(it_cat.mean()),
                                          "qp_iters_p99": float(np.percentile(it_cat, 99)),
                                          "nodes_max": int(np.concatenate(nodes_all).max()) if nodes_all else int(stats["nodes"].max()),
                                          "staged_rows_max_last_round": int(stats["cand"].max())},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_replan": B, "kernel": "k_replan", "kernel_source_sha16": src_sha,
                         "after_prefilter": after},
            "cpu_baseline": cpu,
            "cpu_baseline_warm": cpu_warm,
            "parity_on_timed_rounds": parity,
            "secondary_workloads": secondary,
            "solved_replans_per_s": (n_rob * K - fails_timed) / elapsed,
            "second_window": second,
            "single_instance_call": single,
            "ms_per_step_per_rank": per_rank_ms,
            "exchange_ms_p50": None if exchange_ms is None else exchange_ms["p50"],
            "exchange_ms": exchange_ms,
        }
        if cpu is not None:   # which CPU figure is which (neither is a target): the naive cold-started oracle, and its like-for-like neighbour
            cpu["port_variant"] = "oracle-cold: the literal restatement, every instance cold-started, all n_rob planes formed (a correctness oracle, not a tuned solver)"
            cpu["like_for_like"] = None if cpu_warm is None else {
                "value": cpu_warm["value"], "unit": cpu_warm["unit"], "kind": "port-warm",
                "what": "oracle/hdsm_cpu_port.c: the kernel's own algorithm (lazy planes, prefilter, pick rule, warm start) as scalar C on all host "
                        "cores - the CPU neighbour to compare the GPU figure with (see cpu_baseline_warm)"}
            line["gpu_over_cpu"] = {"vs_cpu_baseline_oracle_cold": value / cpu["value"],
                                    "vs_cpu_baseline_warm": None if cpu_warm is None else value / cpu_warm["value"]}
    # ---------------------------------------------------------------- N > 1: the device-resident loop over RCCL, LAST and under a watchdog
    # Every rank runs hdsm_dswarm_round (its all-gather inside) for K rounds. If the pass does not come back within its budget, rank 0
    # prints the line without it and every rank leaves: the secondary record can cost the line nothing but those seconds.
    if world > 1 and comm is not None and not args.no_event_pass and not args.load_recording:
        import threading
        done = threading.Event()
        budget_s = float(os.environ.get("HDSM_BENCH_DLOOP_BUDGET_S", "90"))

        def watchdog():
            if not done.wait(budget_s):
                if rank == 0:
                    line["device_resident_loop"] = {"error": f"no answer within {budget_s:g} s (pass abandoned; the line above it is complete)", "ranks": world}
                    print(json.dumps(line), flush=True)
                os._exit(0)

        th = threading.Thread(target=watchdog, daemon=True)
        th.start()
        try:
            res = device_loop_pass()
            if rank == 0:
                line["device_resident_loop"] = res
        except BaseException as e:  # noqa: BLE001 (a secondary record)
            if rank == 0:
                line["device_resident_loop"] = {"error": repr(e)[:300], "ranks": world}
        done.set()
    if rank == 0:
        print(json.dumps(line), flush=True)
    if comm is not None:
        comm.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
