"""What the flight audit costs per round of the device-resident loop, on the GPU.

Three set-ups, each one flight in one process: after a warm-up, blocks of rounds with the audit off and on ALTERNATE (the same
swarm, so both see the same phase of the flight); a block is timed on the host from its first launch to the device's idle
(milliseconds per round = block time / rounds). Per set-up: the per-block figures, their median and spread (min, max) for off and
on, and — from a last pass with phase timing on — the medians of hdsm_dswarm_last_audit_ms and of the k_commit phase.
  free   1024 agents, circular exchange in free space, horizon 10
  cfg3   cfg 3's pre-processed forest, 256 agents, horizon 10
  cfg5   cfg 5's pre-processed forest-wall-forest, 4096 agents on a 64 x 64 lattice, 66 x 66 x 40 local grids, horizon 15
The off figure is the yardstick: it is the loop of a build without the audit. Every step runs under its own time limit (an
interval timer whose signal ends the process, also inside a native call), and nothing is tried twice.

usage: python scripts/gpu_flight_audit_timing.py [--steps free,cfg3,cfg5] [--out profiles/flight_audit_timing.json]
       python scripts/gpu_flight_audit_timing.py --fly off|on --steps free [--rounds 40]     (a plain flight, for a kernel trace)
       python scripts/gpu_flight_audit_timing.py --baseline   (the same blocks with no audit call at all; it needs nothing of the
                                                               audit, so this file also runs in a checkout of the commit before it:
                                                               that commit's figure and spread, the yardstick of the off figure)
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_agent_pkgs_amd import lib, swarm  # noqa: E402
from multi_agent_pkgs_amd import scenarios as sc  # noqa: E402
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config, default_map_config  # noqa: E402


class limit:
    """`with limit(s):` — SIGALRM's default action ends the process after s seconds."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)


def preprocessed(raw):
    return lib.map_preprocess(default_map_config(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4),
                              np.ascontiguousarray(raw, np.int8)[None])[0]


def device_swarm(horizon, n_rob, world=None, origin=None, starts=None, goals=None, tall=False):
    prm = agile_params(horizon, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    if tall:
        cfg.grid_range[2], cfg.grid_z_min = 12.0, -6.0
    sol = lib.Solver(prm, n_rob, n_rob)
    rcfg = agile_ref_config()

    def solve(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def ref_dev(ids, path, n_path, plans, has, vel_cap=None):
        full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    loop = swarm.SwarmLoop(prm, cfg, n_rob, solve=solve, reference=ref_dev, starts=starts, goals=goals)
    if world is not None:
        assert loop.set_world(world, origin) == 0
    return loop, swarm.DeviceSwarm(loop.shard, sol)


def make(step):
    if step == "free":
        return device_swarm(10, 1024), 10
    if step == "cfg3":
        raw, origin = sc.forest_for_circle(256, seed=13)
        return device_swarm(10, 256, preprocessed(raw), origin), 10
    n_y = 64
    starts, goals = sc.lattice_scenario(n_y, n_y)
    raw, origin = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
    return device_swarm(15, n_y * n_y, preprocessed(raw), origin, starts=starts, goals=goals, tall=True), 5


def block_ms(dsw, rounds):
    dsw.path_stats()                                   # (synchronises: the block starts on an idle device)
    t0 = time.perf_counter()
    for _ in range(rounds):
        dsw.round()
    dsw.path_stats()
    return (time.perf_counter() - t0) * 1e3 / rounds


def measure_baseline(step, alternations=6):
    """The blocks of measure() with no audit call: warm-up, then 2 x alternations blocks."""
    (loop, dsw), rounds = make(step)
    for _ in range(rounds + 3):
        dsw.round()
    v = [block_ms(dsw, rounds) for _ in range(2 * alternations)]
    dsw.close()
    return dict(agents=loop.n_rob, rounds_per_block=rounds, ms_per_round=dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)),
                                                                              blocks=[float(x) for x in v]))


def measure(step, alternations=6):
    (loop, dsw), rounds = make(step)
    for _ in range(rounds):                            # warm-up, the audit's first launches included
        dsw.round()
    dsw.set_audit(True)
    for _ in range(3):
        dsw.round()
    off, on = [], []
    for _ in range(alternations):
        dsw.set_audit(False)
        off.append(block_ms(dsw, rounds))
        dsw.set_audit(True)
        on.append(block_ms(dsw, rounds))
    dsw.set_phase_timing(True)
    audit_ms, commit_ms, solve_ms = [], [], []
    for _ in range(rounds):
        dsw.round()
        audit_ms.append(dsw.last_audit_ms())
        ph = dsw.phase_ms()
        commit_ms.append(ph["k_commit"]), solve_ms.append(ph["hdsm_replan_device"])
    summ = swarm.flight_summary(dsw.flight_report())
    dsw.close()
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])
    return dict(agents=loop.n_rob, rounds_per_block=rounds, alternations=alternations, ms_per_round_audit_off=stat(off),
                ms_per_round_audit_on=stat(on), last_audit_ms_median=float(np.median(audit_ms)), k_commit_ms_median=float(np.median(commit_ms)),
                replan_ms_median=float(np.median(solve_ms)), flight=summ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="free,cfg3,cfg5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flight_audit_timing.json"))
    ap.add_argument("--fly", choices=("off", "on"))
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    steps = args.steps.split(",")
    if args.fly:
        with limit(400):
            (loop, dsw), _ = make(steps[0])
            if args.fly == "on":
                dsw.set_audit(True)
            for _ in range(args.rounds):
                dsw.round()
            print("flown", steps[0], args.fly, args.rounds, "failed so far", dsw.download(states=False)[3], flush=True)
            dsw.close()
        return
    res = dict(method="host clock over blocks of rounds between two device synchronisations, audit off / on alternated on one flight "
                      "after a warm-up; last_audit_ms and k_commit: HIP events of a last pass with phase timing on")
    for step in steps:
        with limit(500):
            res[step] = measure_baseline(step) if args.baseline else measure(step)
        print(step, json.dumps({k: v for k, v in res[step].items() if k != "flight"}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
