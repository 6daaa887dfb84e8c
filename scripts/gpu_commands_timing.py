"""What the commands for the vehicle (k_command) cost a round of the device-resident loop, on the GPU.

Two flights, each flown once from its start in one process with phase timing on: BASELINE cfg 4's device loop (1024 agents, circle
exchange, free space, H = 10) and cfg 3's pre-processed forest (256 agents, H = 10). After a warm-up the rounds come in alternated
blocks — commands off / on / off / on ... on ONE flight (commands do not steer, so both kinds of block fly the same flight) — and per
block the median over its rounds of entry [5] of hdsm_dswarm_last_phase_ms (k_commit, and k_command behind it) and of the seven
entries summed. Expectation written down before the run: k_command is one more launch of one lane per agent inside entry [5], no
memory traffic to speak of (an agent reads about 1 KB and writes 256 bytes): the few microseconds of a dependent launch,
as k_track; with commands off nothing is launched and the figures are the parent commit's.

--tree DIR flies the same flights with the package of another checkout (the parent commit, built: the yardstick of "off" on the same
device in the same visit) in fresh processes, every block "off", and adds its figures under "parent"; --alternate K repeats that K
times for each checkout, alternated, since one process lies further from the next than one block from the next. "Off" agrees with
the parent when this build's median of process medians lies inside the range of the parent's processes.

--bench K runs `bench.py --gpus 1 --steps 20 --warmup 5` of both checkouts K times each, alternated process by process, and records
ms_per_step of every run with the ranges.

usage: python scripts/gpu_commands_timing.py [--out profiles/commands_timing.json] [--tree DIR [--alternate K] [--bench K]]
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
WARMUP, BLOCK, ALTERNATIONS = 6, 8, 5
FLIGHTS = ("free_1024", "cfg3_forest_256")


def make(tree, flight):
    sys.path.insert(0, tree)
    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params, agile_ref_config, default_map_config

    prm, cfg = agile_params(10, max_rows_static=18), swarm.default_swarm_config()
    if flight == "free_1024":
        n = 1024
        starts, goals = sc.circle_scenario(n)
        sol = lib.Solver(prm, n, n)
        return sol, swarm.DeviceSwarm(swarm.SwarmShard(prm, cfg, n, 0, starts, goals), sol)
    n = 256
    raw, origin = sc.forest_for_circle(n, seed=13)
    world = lib.map_preprocess(default_map_config(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4),
                               np.ascontiguousarray(raw, np.int8)[None])[0]
    sol, rcfg = lib.Solver(prm, n, n), agile_ref_config()

    def solve(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def ref_dev(ids, path, n_path, plans, has, vel_cap=None):
        full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    loop = swarm.SwarmLoop(prm, cfg, n, solve=solve, reference=ref_dev)
    assert loop.set_world(world, origin) == 0
    return sol, swarm.DeviceSwarm(loop.shard, sol)


def measure(tree, flight, commands):
    """The blocks of one flight: `commands` False flies every block off and calls nothing of the feature (any checkout)."""
    sol, dsw = make(tree, flight)
    dsw.set_phase_timing(True)
    for _ in range(WARMUP):
        dsw.round()
    blocks = []
    for b in range(2 * ALTERNATIONS):
        on = commands and b % 2 == 1
        if commands:
            dsw.set_commands(on)
        commit, whole = [], []
        for _ in range(BLOCK):
            dsw.round()
            ms = dsw.phase_ms()
            commit.append(ms["k_commit"]), whole.append(sum(ms.values()))
        blocks.append(dict(commands="on" if on else "off", phase5_ms_median=float(np.median(commit)), round_ms_median=float(np.median(whole)),
                           phase5_ms=[float(x) for x in commit]))
    out = dict(blocks=blocks, no_solution_so_far=int(dsw.download(states=False)[3]))
    if commands:
        out["command_stats"] = dsw.command_stats()
    for key in ("phase5_ms_median", "round_ms_median"):
        for kind in ("off", "on") if commands else ("off",):
            v = [blk[key] for blk in blocks if blk["commands"] == kind]
            out[f"{key}_{kind}"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    dsw.close(), sol.close()
    return out


def child(args_):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_, capture_output=True, text=True, timeout=400, check=True).stdout
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])


def bench_line(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                         timeout=400, check=True, cwd=tree).stdout
    line = next(ln for ln in reversed(out.splitlines()) if ln.startswith("{"))
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commands_timing.json"))
    ap.add_argument("--tree", default=None, help="another built checkout (the parent commit): its 'off' blocks are measured in fresh processes")
    ap.add_argument("--alternate", type=int, default=0, help="with --tree: K fresh processes of each checkout, alternated, every block off")
    ap.add_argument("--bench", type=int, default=0, help="with --tree: K runs of the bench line of each checkout, alternated")
    ap.add_argument("--off-only", default="", help="(a child process) print the all-off blocks of this flight with the package of --tree")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)        # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 1100)
    if args.off_only:
        print("RESULT " + json.dumps(measure(os.path.abspath(args.tree), args.off_only, False)), flush=True)
        return
    res = dict(method=f"per flight one process: {WARMUP} warm-up rounds, then {2 * ALTERNATIONS} blocks of {BLOCK} phase-timed rounds, commands off / on "
                      "alternated on the one flight; per block the median of entry [5] of hdsm_dswarm_last_phase_ms (k_commit + k_command) and of the "
                      "seven entries summed; per kind the median, minimum and maximum over its blocks",
               expectation="k_command is one more dependent launch inside entry [5]: a few microseconds, as k_track; off launches nothing", flights={})
    for flight in FLIGHTS:
        res["flights"][flight] = m = measure(ROOT, flight, True)
        m["cost_ms"] = {key: m[f"{key}_on"]["median"] - m[f"{key}_off"]["median"] for key in ("phase5_ms_median", "round_ms_median")}
        print(flight, json.dumps({k: v for k, v in m.items() if k != "blocks"}), flush=True)
    if args.tree:
        tree = os.path.abspath(args.tree)
        for flight in FLIGHTS:
            alt = dict(this=[], parent=[])
            for _ in range(max(1, args.alternate)):
                for name, t in (("this", ROOT), ("parent", tree)):
                    r = child(["--off-only", flight, "--tree", t])
                    alt[name].append({key: r[f"{key}_off"]["median"] for key in ("phase5_ms_median", "round_ms_median")})
            summ = dict(processes=alt)
            for key in ("phase5_ms_median", "round_ms_median"):
                a, b = [x[key] for x in alt["this"]], [x[key] for x in alt["parent"]]
                summ[key] = dict(this_median=float(np.median(a)), this_range=[min(a), max(a)], parent_median=float(np.median(b)), parent_range=[min(b), max(b)],
                                 off_inside_parent_spread=bool(min(b) <= float(np.median(a)) <= max(b)))
            res["flights"][flight]["off_against_parent"] = summ
            print(flight, "off against parent", json.dumps({k: v for k, v in summ.items() if k != "processes"}), flush=True)
        if args.bench > 0:
            runs = dict(this_build=[], commit_before=[])
            t0 = time.time()
            for _ in range(args.bench):
                for name, t in (("this_build", ROOT), ("commit_before", tree)):
                    runs[name].append(bench_line(t))
                print("bench", json.dumps(runs), f"{time.time() - t0:.0f} s", flush=True)
            res["bench_line"] = dict(command="bench.py --gpus 1 --steps 20 --warmup 5", ms_per_step=runs,
                                     median={k: float(np.median(v)) for k, v in runs.items()}, range={k: [min(v), max(v)] for k, v in runs.items()})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
