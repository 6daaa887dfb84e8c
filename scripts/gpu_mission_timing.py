"""What a mission (k_mission, the device-sized path launch, hdsm_dswarm_fly) costs the device-resident loop, on the GPU.

cost      Circle flights of 64 and 1024 agents in free space (H = 10), each flown once in one process with phase timing on. After a
          warm-up the rounds come in alternated blocks — mission off / on, --repeats times — on ONE flight; per block the median over
          its rounds of entry [5] of hdsm_dswarm_last_phase_ms (k_commit and, behind it, k_mission) and of a host clock round the
          round (issue + synchronise). The mission's one waypoint per agent is the agent's goal, so "on" steers nobody anywhere else;
          with the mission on the path step is one more launch (device-sized, nobody due).
empty     The device-sized path launch in rounds where nobody is due: 256 agents in cfg 3's forest (--big: and the 4096 agents of
          cfg 5's lane forest), path period 0, k_path and k_dmp (clearance 1.8): blocks off / on alternated, the host clock round the
          round and, for the "on" blocks, hdsm_dswarm_last_path_ms (the launch alone). Every block, off or on, follows one untimed
          round in which everybody planned, so that both kinds fly on equally fresh paths.
fly       hdsm_dswarm_fly with check_every 1, 4, 16 against a Python loop of round() on the 1024-agent circle, milliseconds per round
          over 64 rounds from the same start (the waypoints are not reached in them). Report only.
--tree DIR flies the cost flights with the package of another checkout (the parent commit, built) in fresh processes, nothing of the
          feature called, alternated with this build --alternate K times, and --bench K runs `bench.py --gpus 1 --steps 20 --warmup 5`
          of both checkouts K times each, alternated: "off" agrees with the parent when this build's median of process medians lies
          inside the range of the parent's processes.

EXPECTATION, written down before the run: k_mission is one more dependent launch inside entry [5] — a launch's latency, a few
microseconds, the same at 64 and 1024 agents; an empty device-sized path launch is a launch whose workgroups return at once: a
launch's latency for 256 agents, and for k_dmp at 4096 agents sixteen waves of empty workgroups on top.

usage: python scripts/gpu_mission_timing.py [--out profiles/mission_timing.json] [--big] [--tree DIR [--alternate K] [--bench K]]
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
WARMUP, BLOCK = 6, 8
FLIGHTS = dict(free_1024=1024, circle_64=64)


def modules(tree):
    sys.path.insert(0, tree)
    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params
    return lib, swarm, sc, agile_params(10, max_rows_static=18)


def circle(tree, n):
    lib, swarm, sc, prm = modules(tree)
    starts, goals = sc.circle_scenario(n)
    sol = lib.Solver(prm, n, n)
    return sol, swarm.DeviceSwarm(swarm.SwarmShard(prm, swarm.default_swarm_config(), n, 0, starts, goals), sol), sc, goals


def forest(tree, n, clearance, big):
    lib, swarm, sc, prm = modules(tree)
    if big:
        starts, goals, world, origin = sc.lane_forest_scenario(64, 64)      # (inflated already)
    else:
        starts, goals = sc.circle_scenario(n)
        raw, origin = sc.forest_for_circle(n, seed=21)
        world = sc.inflate(raw)
    n = len(starts)
    shard = swarm.SwarmShard(prm, swarm.default_swarm_config(), n, 0, starts, goals)
    shard.set_world(world, origin)
    if clearance:
        shard.set_path_clearance(clearance)
    shard.set_path_period(0)
    sol = lib.Solver(prm, n, n)
    return sol, swarm.DeviceSwarm(shard, sol), sc, goals


def _block(dsw, sync, path_ms=False):
    commit, whole, path = [], [], []
    for _ in range(BLOCK):
        t0 = time.perf_counter()
        dsw.round()
        ms = dsw.phase_ms()                                  # (synchronises with the round)
        whole.append(1e3 * (time.perf_counter() - t0)), commit.append(ms["k_commit"])
        if path_ms:
            path.append(dsw.last_path_ms())
    out = dict(phase5_ms=float(np.median(commit)), round_ms=float(np.median(whole)))
    if path_ms:
        out["path_ms"] = float(np.median(path))
    return out


def _fold(blocks, keys):
    out = {}
    for kind in ("off", "on"):
        mine = [b for b in blocks if b["kind"] == kind]
        for key in keys:
            v = [b[key] for b in mine if key in b]
            if v:
                out[f"{key}_{kind}"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    return out


def measure(tree, make, repeats, mission, path_ms=False):
    """The blocks of one flight: `mission` False flies every block off and calls nothing of the feature (any checkout)."""
    sol, dsw, sc, goals = make()
    dsw.set_phase_timing(True)
    for _ in range(WARMUP):
        dsw.round()
    blocks = []
    for b in range(2 * repeats):
        on = mission and b % 2 == 1
        if mission:
            # Every block, off or on, starts behind the same thing: the mission set and ONE round flown in which everybody is due and
            # plans (not timed). New paths leave the corridor's polyhedron cache cold for some rounds; a block that follows a replanning
            # must be compared with a block that follows one. The off blocks then switch the mission off again.
            dsw.set_mission(sc.mission_setting(1), goals[:, None, :])
            dsw.round()
            if not on:
                dsw.set_mission(None)
        blocks.append(dict(_block(dsw, None, path_ms=path_ms and on), kind="on" if on else "off"))
    out = dict(blocks=blocks, **_fold(blocks, ("phase5_ms", "round_ms", "path_ms")))
    if mission:
        out["mission_stats"], out["path_stats"] = dsw.mission_stats(), dsw.path_stats()
        out["cost_us"] = {k: 1e3 * (out[f"{k}_on"]["median"] - out[f"{k}_off"]["median"]) for k in ("phase5_ms", "round_ms")}
    dsw.close(), sol.close()
    return out


def fly_report(rounds=64):
    out = {}
    for name, every in (("python_loop", 0), ("fly_check_every_1", 1), ("fly_check_every_4", 4), ("fly_check_every_16", 16)):
        sol, dsw, sc, goals = circle(ROOT, 1024)
        dsw.set_mission(sc.mission_setting(1), goals[:, None, :])
        for _ in range(WARMUP):
            dsw.round()
        dsw.mission_summary()                                # (synchronises)
        t0 = time.perf_counter()
        if every:
            flown, last = dsw.fly(rounds, check_every=every)
        else:
            for _ in range(rounds):
                dsw.round()
            flown, last = rounds, dsw.mission_summary()
        out[name] = dict(ms_per_round=1e3 * (time.perf_counter() - t0) / flown, rounds=flown, done=last["done"])
        dsw.close(), sol.close()
    return out


def child(args_):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_, capture_output=True, text=True, timeout=400, check=True).stdout
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])


def bench_line(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                         timeout=400, check=True, cwd=tree).stdout
    return float(json.loads(next(ln for ln in reversed(out.splitlines()) if ln.startswith("{")))["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mission_timing.json"))
    ap.add_argument("--repeats", type=int, default=4, help="off / on pairs of blocks per flight")
    ap.add_argument("--big", action="store_true", help="also the 4096 agents of cfg 5's lane forest for the empty path launch")
    ap.add_argument("--tree", default=None, help="another built checkout (the parent commit): its 'off' blocks are measured in fresh processes")
    ap.add_argument("--alternate", type=int, default=0, help="with --tree: K fresh processes of each checkout, alternated, every block off")
    ap.add_argument("--bench", type=int, default=0, help="with --tree: K runs of the bench line of each checkout, alternated")
    ap.add_argument("--skip-flights", action="store_true", help="only what --tree asks for")
    ap.add_argument("--off-only", default="", help="(a child process) print the all-off blocks of this flight with the package of --tree")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)            # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 1100)
    if args.off_only:
        tree = os.path.abspath(args.tree)
        print("RESULT " + json.dumps(measure(tree, lambda: circle(tree, FLIGHTS[args.off_only]), 4, False)), flush=True)
        return
    res = dict(method=f"{WARMUP} warm-up rounds, then off / on blocks of {BLOCK} phase-timed rounds alternated on one flight; per block the median of entry "
                      "[5] of hdsm_dswarm_last_phase_ms and of a host clock round issue + synchronise; per kind the median, minimum and maximum over "
                      "its blocks; cost_us = median on - median off",
               expectation="k_mission: one more dependent launch in entry [5], a few microseconds, the same at 64 and 1024 agents; an empty device-sized "
                           "path launch: a launch's latency at 256 agents, sixteen waves of empty workgroups on top for k_dmp at 4096",
               notes="every block, off or on, follows one untimed round in which everybody planned (the mission set; switched off again for an "
                     "off block), so both kinds fly on equally fresh paths; round_ms is a host clock round issue + synchronise and carries the "
                     "host's jitter — at 64 agents and in the forests it moves by more between blocks of one kind than between the kinds, so "
                     "its cost_us is noise there: the figures to read are phase5_ms (HIP events) and path_ms (the path launch alone)",
               cost={}, empty_path_launch={})
    if not args.skip_flights:
        for flight, n in FLIGHTS.items():
            res["cost"][flight] = m = measure(ROOT, lambda n=n: circle(ROOT, n), args.repeats, True)
            print(flight, json.dumps({k: v for k, v in m.items() if k != "blocks"}), flush=True)
        worlds = [("forest_256", 256, False)] + ([("lane_forest_4096", 4096, True)] if args.big else [])
        for name, n, big in worlds:
            for kernel, clearance in (("k_path", 0.0), ("k_dmp", 1.8)):
                res["empty_path_launch"][f"{name}_{kernel}"] = m = measure(ROOT, lambda n=n, c=clearance, b=big: forest(ROOT, n, c, b), args.repeats, True,
                                                                           path_ms=True)
                print(name, kernel, json.dumps({k: v for k, v in m.items() if k != "blocks"}), flush=True)
        res["fly_1024_agents"] = fly_report()
        print("fly", json.dumps(res["fly_1024_agents"]), flush=True)
    if args.tree:
        tree = os.path.abspath(args.tree)
        res["off_against_parent"] = {}
        for flight in FLIGHTS if args.alternate > 0 else ():
            alt = dict(this=[], parent=[])
            for _ in range(args.alternate):
                for name, t in (("this", ROOT), ("parent", tree)):
                    r = child(["--off-only", flight, "--tree", t])
                    alt[name].append({key: r[f"{key}_off"]["median"] for key in ("phase5_ms", "round_ms")})
            summ = dict(processes=alt)
            for key in ("phase5_ms", "round_ms"):
                a, b = [x[key] for x in alt["this"]], [x[key] for x in alt["parent"]]
                summ[key] = dict(this_median=float(np.median(a)), this_range=[min(a), max(a)], parent_median=float(np.median(b)), parent_range=[min(b), max(b)],
                                 off_inside_parent_range=bool(min(b) <= float(np.median(a)) <= max(b)))
            res["off_against_parent"][flight] = summ
            print(flight, "off against parent", json.dumps({k: v for k, v in summ.items() if k != "processes"}), flush=True)
        if args.bench > 0:
            runs = dict(this_build=[], commit_before=[])
            for _ in range(args.bench):
                for name, t in (("this_build", ROOT), ("commit_before", tree)):
                    runs[name].append(bench_line(t))
                print("bench", json.dumps(runs), flush=True)
            res["off_against_parent"]["bench"] = dict(command="bench.py --gpus 1 --steps 20 --warmup 5, alternated process by process", ms_per_step=runs,
                                                      median={k: float(np.median(v)) for k, v in runs.items()},
                                                      range={k: [min(v), max(v)] for k, v in runs.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
