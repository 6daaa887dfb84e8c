"""What neighbour groups buy: many small swarms in one flight of the device-resident loop, on the GPU.

Two set-ups — 256 swarms of 16 agents (4096 agents) and 410 swarms of 10 (4100) — each a circular exchange in free space with
horizon 10 and the flight audit on. Each is flown twice in one process:
  grouped   every swarm at the SAME coordinates, one neighbour group per swarm (hdsm_swarm_set_groups -> hdsm_dswarm_create);
  tiled     the only thing a build without groups can do: the same swarms 1 km apart in one frame, no partition — every agent
            stays a neighbour of every other one (reference speeds, sweeps over all spheres, all pairs in the audit).
After a warm-up, blocks of rounds of the two flights ALTERNATE (both see the same phase of the flight); a block is timed on the
host from its first launch to the device's idle (milliseconds per round = block time / rounds). A last pass with phase timing on
gives the medians of the reference, solver and audit phases (HIP events between the launches). Every set-up runs under its own
time limit (an interval timer whose signal ends the process, also inside a native call), and nothing is tried twice.

usage: python scripts/gpu_groups_timing.py [--steps 256x16,410x10] [--out profiles/groups_timing.json]
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
from multi_agent_pkgs_amd.params import agile_params  # noqa: E402

HORIZON, RADIUS, TILE = 10, 8.0, (1000.0, 0.0, 0.0)


class limit:
    """`with limit(s):` — SIGALRM's default action ends the process after s seconds."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)


def flight(copies, size, grouped):
    prm = agile_params(HORIZON, max_rows_static=18)
    s1, g1 = sc.circle_scenario(size, radius=RADIUS)
    starts, goals, groups = sc.repeat_scenario(s1, g1, copies, offset=(0.0, 0.0, 0.0) if grouped else TILE)
    n = starts.shape[0]
    sol = lib.Solver(prm, n, n)
    shard = swarm.SwarmShard(prm, swarm.default_swarm_config(), n, 0, starts, goals)
    if grouped:
        shard.set_groups(groups)
    shard.set_audit(True, 1.0)
    return sol, shard, swarm.DeviceSwarm(shard, sol)


def block_ms(dsw, rounds):
    dsw.path_stats()                                   # (synchronises: the block starts on an idle device)
    t0 = time.perf_counter()
    for _ in range(rounds):
        dsw.round()
    dsw.path_stats()
    return (time.perf_counter() - t0) * 1e3 / rounds


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])


def measure(copies, size, warm=5, rounds=4, alternations=5):
    flights = {"grouped": flight(copies, size, True), "tiled": flight(copies, size, False)}
    for _, _, dsw in flights.values():
        for _ in range(warm):
            dsw.round()
    per_round = {k: [] for k in flights}
    for _ in range(alternations):
        for k, (_, _, dsw) in flights.items():
            per_round[k].append(block_ms(dsw, rounds))
    phases = {k: dict(reference=[], solver=[], audit=[]) for k in flights}
    for _, _, dsw in flights.values():
        dsw.set_phase_timing(True)
    for _ in range(rounds):
        for k, (_, _, dsw) in flights.items():
            dsw.round()
            ph = dsw.phase_ms()
            phases[k]["reference"].append(ph["hdsm_reference_device"]), phases[k]["solver"].append(ph["hdsm_replan_device"])
            phases[k]["audit"].append(dsw.last_audit_ms())
    res = dict(swarms=copies, agents_per_swarm=size, agents=copies * size, horizon=HORIZON, warm_up_rounds=warm, rounds_per_block=rounds,
               alternations=alternations)
    for k, (sol, shard, dsw) in flights.items():
        _, _, status, failed = dsw.download(states=False)
        res[k] = dict(ms_per_round=stat(per_round[k]), phase_ms_median={p: float(np.median(v)) for p, v in phases[k].items()},
                      no_solution_last_round=int((status == 2).sum()), no_solution_so_far=int(failed),
                      flight=swarm.flight_summary(dsw.flight_report()))
        dsw.close(), sol.close()
    res["grouped_over_tiled"] = dict(ms_per_round=res["grouped"]["ms_per_round"]["median"] / res["tiled"]["ms_per_round"]["median"],
                                     **{p: res["grouped"]["phase_ms_median"][p] / max(res["tiled"]["phase_ms_median"][p], 1e-9)
                                        for p in ("reference", "solver", "audit")})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="256x16,410x10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_timing.json"))
    args = ap.parse_args()
    res = dict(method="host clock over blocks of rounds between two device synchronisations, the grouped and the tiled flight alternated in one "
                      "process after a warm-up; phases: HIP events of a last pass with phase timing on (medians)")
    for step in args.steps.split(","):
        copies, size = (int(x) for x in step.split("x"))
        with limit(400):
            res[step] = measure(copies, size)
        print(step, json.dumps({k: v for k, v in res[step].items() if k not in ("grouped", "tiled")}),
              json.dumps({k: {f: v for f, v in res[step][k].items() if f != "flight"} for k in ("grouped", "tiled")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
