"""What local ranks cost on ONE device: the sharded device loop of hdsm_dswarm_round_ranks next to the plain round, on the GPU.

1024 agents, circular exchange in free space, horizon 10. The same swarm is flown as world = 1 (hdsm_dswarm_round on one rank, no
communicator: the yardstick) and as 2, 4 and 8 local ranks on the one device, every rank on a stream of its own. After a warm-up,
blocks of rounds of the flights ALTERNATE (all see the same phase of the flight); a block is timed on the host from its first launch
to the device's idle, all ranks together (milliseconds per round = block time / rounds). A last pass with phase timing on gives
entry [6] of hdsm_dswarm_last_phase_ms — the rank's k_gather_local — and the solve, per rank and round (HIP events on the rank's
stream). The process runs under one time limit (an interval timer whose signal ends it, also inside a native call); nothing is tried
twice.

Expectation, written down before the first run: the gather costs a launch, 3 to 5 us per rank; the round on one device gets no
faster with `world`, because the ranks share the CUs and each solves a smaller batch in a shape chosen for it. Figures for more than
one device are not produced here.

usage: python scripts/gpu_local_ranks_timing.py [--agents 1024] [--worlds 1,2,4,8] [--out profiles/local_ranks_timing.json]
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

HORIZON = 10


class Plain:
    """world = 1: one DeviceSwarm flown by hdsm_dswarm_round."""

    def __init__(self, prm, cfg, starts, goals):
        n = starts.shape[0]
        self.world = 1
        self.sol = lib.Solver(prm, n, n)
        self.shard = swarm.SwarmShard(prm, cfg, n, 0, starts, goals)
        self.dswarms = [swarm.DeviceSwarm(self.shard, self.sol)]

    def round(self):
        self.dswarms[0].round()

    def close(self):
        self.dswarms[0].close(), self.sol.close()


class Ranks:
    """world > 1: swarm.LocalRanks on device 0, a stream per rank."""

    def __init__(self, prm, cfg, starts, goals, world):
        import torch
        self.world = world
        self.ranks = swarm.LocalRanks(prm, cfg, starts.shape[0], world, starts=starts, goals=goals)
        self.dswarms = self.ranks.dswarms
        self.streams = [torch.cuda.Stream() for _ in range(world)]

    def round(self):
        self.ranks.round(self.streams)

    def close(self):
        self.ranks.close()


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])


def measure(n_agents, worlds, warm=5, rounds=4, alternations=5):
    import torch
    prm, cfg = agile_params(HORIZON, max_rows_static=18), swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(n_agents)
    flights = {w: (Plain(prm, cfg, starts, goals) if w == 1 else Ranks(prm, cfg, starts, goals, w)) for w in worlds}
    for f in flights.values():
        for _ in range(warm):
            f.round()
    torch.cuda.synchronize()
    per_round = {w: [] for w in worlds}
    for _ in range(alternations):
        for w, f in flights.items():
            torch.cuda.synchronize()                 # the block starts on an idle device
            t0 = time.perf_counter()
            for _ in range(rounds):
                f.round()
            torch.cuda.synchronize()
            per_round[w].append((time.perf_counter() - t0) * 1e3 / rounds)
    gather, solve, commit = ({w: [] for w in worlds} for _ in range(3))
    for f in flights.values():
        for d in f.dswarms:
            d.set_phase_timing(True)
    for _ in range(rounds):
        for w, f in flights.items():
            f.round()
            for d in f.dswarms:
                ph = d.phase_ms()
                gather[w].append(ph["exchange"]), solve[w].append(ph["hdsm_replan_device"]), commit[w].append(ph["k_commit"])
    res = dict(agents=n_agents, horizon=HORIZON, warm_up_rounds=warm, rounds_per_block=rounds, alternations=alternations, worlds={})
    for w, f in flights.items():
        failed = sum(d.download(states=False)[3] for d in f.dswarms)
        res["worlds"][str(w)] = dict(ranks=w, agents_per_rank=(n_agents + w - 1) // w, ms_per_round_all_ranks=stat(per_round[w]),
                                     gather_ms_per_rank=stat(gather[w]), solve_ms_per_rank=stat(solve[w]),
                                     commit_and_wait_ms_per_rank=stat(commit[w]), no_solution_so_far=int(failed))
        f.close()
    base = res["worlds"][str(worlds[0])]["ms_per_round_all_ranks"]["median"]
    res["round_over_first_world"] = {str(w): res["worlds"][str(w)]["ms_per_round_all_ranks"]["median"] / base for w in worlds}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ranks_timing.json"))
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.setitimer(signal.ITIMER_REAL, 400)        # SIGALRM's default action ends the process
    res = dict(method="host clock over blocks of rounds between two device synchronisations, all ranks of a world size together, the world "
                      "sizes alternated in one process after a warm-up, all ranks on device 0 with a stream each; gather / solve / commit: "
                      "HIP events of a last pass with phase timing on, per rank and round ([6], [4], [5] of hdsm_dswarm_last_phase_ms; "
                      "a local rank's [5] holds its wait for the other ranks)",
               expectation="gather 3-5 us per rank (a launch); the round on one device gets no faster with world")
    res.update(measure(args.agents, [int(w) for w in args.worlds.split(",")]))
    signal.setitimer(signal.ITIMER_REAL, 0)
    print(json.dumps({w: {k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()} for w, r in res["worlds"].items()}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
