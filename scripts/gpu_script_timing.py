"""What scripted agents cost a round of the device-resident loop, on the GPU.

The flight: 1024 agents, circle exchange, free space, H = 10 — flown twice in one process, unscripted and with the last 32 ids
scripted (each on a line track from its start to its goal at 3 m/s, predict = 1). After a warm-up, blocks of rounds of the two
flights alternate; a block is timed on the host between two device synchronisations. A last pass with phase timing on gives entry
[5] of hdsm_dswarm_last_phase_ms (k_commit, and k_script behind it) of the same rounds. Expectation written down before the run:
k_script costs about a launch — entry [5] grows by a few microseconds, and the whole round does not grow at all, because 32 agents
fewer are planned for.

--tree DIR flies the unscripted flight alone with the package of another checkout (the parent commit, built, as the yardstick of
the unscripted figure: same device, same visit) in a fresh process and adds its figures under "parent".

usage: python scripts/gpu_script_timing.py [--out profiles/script_timing.json] [--tree DIR]
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGENTS, N_SCRIPT, N_HOR = 1024, 32, 10


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])


def measure(tree, scripted, warm=5, rounds=4, alternations=6):
    sys.path.insert(0, tree)
    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params

    prm = agile_params(N_HOR, max_rows_static=18)
    starts, goals = sc.circle_scenario(N_AGENTS)

    def flight(n_script):
        sol = lib.Solver(prm, N_AGENTS, N_AGENTS)
        dsw = swarm.DeviceSwarm(swarm.SwarmShard(prm, swarm.default_swarm_config(), N_AGENTS, 0, starts, goals), sol)
        if n_script:
            first = N_AGENTS - n_script
            dsw.set_script(np.stack([sc.line_track(starts[k], goals[k], 3.0) for k in range(first, N_AGENTS)]), 1)
        return sol, dsw

    def block_ms(dsw):
        dsw.path_stats()                                 # (synchronises: the block starts on an idle device)
        t0 = time.perf_counter()
        for _ in range(rounds):
            dsw.round()
        dsw.path_stats()
        return (time.perf_counter() - t0) * 1e3 / rounds

    flights = {str(n): flight(n) for n in ((0, N_SCRIPT) if scripted else (0,))}
    for _, dsw in flights.values():
        for _ in range(warm):
            dsw.round()
    per_round = {k: [] for k in flights}
    for _ in range(alternations):
        for k, (_, dsw) in flights.items():
            per_round[k].append(block_ms(dsw))
    commit = {k: [] for k in flights}
    for _, dsw in flights.values():
        dsw.set_phase_timing(True)
    for _ in range(rounds * alternations):
        for k, (_, dsw) in flights.items():
            dsw.round()
            commit[k].append(dsw.phase_ms()["k_commit"])
    res = dict(agents=N_AGENTS, n_hor=N_HOR, warm_up_rounds=warm, rounds_per_block=rounds, alternations=alternations,
               ms_per_round={k: stat(v) for k, v in per_round.items()}, phase5_ms={k: stat(v) for k, v in commit.items()})
    if scripted:
        res["script_stats"] = flights[str(N_SCRIPT)][1].script_stats()
    for sol, dsw in flights.values():
        dsw.close(), sol.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "script_timing.json"))
    ap.add_argument("--tree", default=None, help="another built checkout: its unscripted flight is measured in a fresh process")
    ap.add_argument("--unscripted-only", action="store_true", help="(the child process of --tree) print the unscripted figures of --tree")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)        # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 540)
    if args.unscripted_only:
        print("RESULT " + json.dumps(measure(os.path.abspath(args.tree), scripted=False)), flush=True)
        return
    res = dict(method="host clock over blocks of rounds between two device synchronisations, 0 and 32 scripted agents alternated in one "
                      "process after a warm-up; phase5_ms: entry [5] of hdsm_dswarm_last_phase_ms (k_commit and, with scripted agents, "
                      "k_script) from HIP events of a last pass with phase timing on",
               expectation="k_script costs about a launch: entry [5] grows by a few microseconds; the round does not grow")
    res.update(measure(ROOT, scripted=True))
    print(json.dumps(res), flush=True)
    if args.tree:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--unscripted-only", "--tree", args.tree], capture_output=True, text=True,
                             timeout=300, check=True).stdout
        res["parent"] = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
        print("parent", json.dumps(res["parent"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
