"""What link faults cost a round of the device-resident loop, and what they do to a flight, on the GPU.

Cost: the same swarm flown twice in one process, links off and links on with an ALL-ZERO table (every record on time: the same
flight, so the difference is k_deliver plus reading the view instead of the plans buffer). After a warm-up, blocks of rounds of the
two flights alternate; a block is timed on the host between two device synchronisations. A last pass with phase timing on gives
k_commit of the same rounds (HIP events), to set the difference against. Two set-ups: 1024 agents in free space at H = 10 (a
circle exchange) and 4096 agents at H = 15 (BASELINE cfg 5's lattice, free space).

Report only: the 1024-agent circle with the audit on, 40 rounds, under 10 % loss and under latency 2, each with time_aware on and
off, next to the perfect link: sigma_min of the flight and the agent-rounds below sigma 1. Expectation written down before the run:
loss and latency LOWER sigma_min (agents decide on positions the others have left), time_aware recovers part of it under pure
latency (a late record advanced by its age is the record a fresh one would have been, if the sender kept to its plan) and helps less
under loss (older records, advanced further, are worse predictions). Nothing here is asserted.

usage: python scripts/gpu_links_timing.py [--out profiles/links_timing.json] [--skip-report]
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


class limit:
    """`with limit(s):` — SIGALRM's default action ends the process after s seconds."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)


def scene(name):
    if name == "circle1024-h10":
        return 10, sc.circle_scenario(1024)
    return 15, sc.lattice_scenario(64, 64)               # 4096 agents, cfg 5's lattice without its forest


def flight(name, audit=False):
    n_hor, (starts, goals) = scene(name)
    prm = agile_params(n_hor, max_rows_static=18)
    n = starts.shape[0]
    sol = lib.Solver(prm, n, n)
    shard = swarm.SwarmShard(prm, swarm.default_swarm_config(), n, 0, starts, goals)
    if audit:
        shard.set_audit(True, 1.0)
    return sol, swarm.DeviceSwarm(shard, sol), n


def block_ms(dsw, rounds):
    dsw.path_stats()                                     # (synchronises: the block starts on an idle device)
    t0 = time.perf_counter()
    for _ in range(rounds):
        dsw.round()
    dsw.path_stats()
    return (time.perf_counter() - t0) * 1e3 / rounds


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])


def cost(name, warm=5, rounds=4, alternations=6):
    flights = {"off": flight(name), "on": flight(name)}
    n = flights["on"][2]
    flights["on"][1].set_links(np.zeros((1, n), np.int8), True)
    for _, dsw, _ in flights.values():
        for _ in range(warm):
            dsw.round()
    per_round = {k: [] for k in flights}
    for _ in range(alternations):
        for k, (_, dsw, _) in flights.items():
            per_round[k].append(block_ms(dsw, rounds))
    commit = {k: [] for k in flights}
    for _, dsw, _ in flights.values():
        dsw.set_phase_timing(True)
    for _ in range(rounds):
        for k, (_, dsw, _) in flights.items():
            dsw.round()
            commit[k].append(dsw.phase_ms()["k_commit"])
    res = dict(agents=n, warm_up_rounds=warm, rounds_per_block=rounds, alternations=alternations,
               ms_per_round={k: stat(v) for k, v in per_round.items()}, k_commit_ms_median={k: float(np.median(v)) for k, v in commit.items()})
    res["on_minus_off_ms"] = res["ms_per_round"]["on"]["median"] - res["ms_per_round"]["off"]["median"]
    res["link_stats"] = flights["on"][1].link_stats()
    for sol, dsw, _ in flights.values():
        dsw.close(), sol.close()
    return res


def report(rounds=40):
    out = {}
    n = 1024
    tables = {"perfect": None, "loss10": sc.link_table(rounds, n, loss=0.10, seed=1), "latency2": sc.link_table(rounds, n, delay_min=2, delay_max=2)}
    for tname, fate in tables.items():
        for aware in ((True,) if fate is None else (True, False)):
            sol, dsw, _ = flight("circle1024-h10", audit=True)
            if fate is not None:
                dsw.set_links(fate, aware)
            for _ in range(rounds):
                dsw.round()
            s = swarm.flight_summary(dsw.flight_report())
            _, _, _, failed = dsw.download(states=False)
            key = tname if fate is None else f"{tname}-{'time_aware' if aware else 'as_is'}"
            out[key] = dict(sigma_min=float(s["sigma_min"]), close_rounds=int(s["close_rounds"]), no_solution_so_far=int(failed),
                            link_stats=dsw.link_stats())
            print(key, json.dumps(out[key]), flush=True)
            dsw.close(), sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links_timing.json"))
    ap.add_argument("--skip-report", action="store_true")
    args = ap.parse_args()
    res = dict(method="host clock over blocks of rounds between two device synchronisations, links off and links on (all-zero table) "
                      "alternated in one process after a warm-up; k_commit: HIP events of a last pass with phase timing on (medians)")
    for name in ("circle1024-h10", "lattice4096-h15"):
        with limit(300):
            res[name] = cost(name)
        print(name, json.dumps(res[name]), flush=True)
    if not args.skip_report:
        with limit(400):
            res["report_circle1024"] = report()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
