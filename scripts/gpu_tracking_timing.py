"""What imperfect tracking (k_track) costs a round of the device-resident loop, on the GPU.

The flight: BASELINE cfg 4's device loop — 1024 agents, circle exchange, free space, H = 10 — flown four times from its start in
one process: tracking model off / on / off / on. Every round runs with phase timing on; per leg the median over rounds 3-12 of
entry [5] of hdsm_dswarm_last_phase_ms (k_commit, and k_track behind it) and of the round (the seven entries summed: the HIP events
of the round's own stream). Expectation written down before the run: k_track is one more small launch inside entry [5], a few
microseconds on a round of about 148 us; with the model off nothing is launched and the figures are the parent commit's.

--tree DIR flies the two "off" legs alone with the package of another checkout (the parent commit, built, as the yardstick of the
"off" figure: same device, same visit) in a fresh process and adds its figures under "parent". The "off" legs agree with the parent
when their medians differ from its by no more than the two "off" legs differ from each other (and the parent's own two).

--alternate K adds K fresh processes of each checkout, this one and --tree's, alternated, each flying the two "off" legs: how far
one process lies from the next with the same code, which the one-process comparison cannot show.

usage: python scripts/gpu_tracking_timing.py [--out profiles/tracking_timing.json] [--tree DIR [--alternate K]]
"""
import argparse
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGENTS, N_HOR, ROUNDS, FIRST = 1024, 10, 13, 3


def measure(tree, legs):
    sys.path.insert(0, tree)
    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params

    prm = agile_params(N_HOR, max_rows_static=18)
    starts, goals = sc.circle_scenario(N_AGENTS)
    out = []
    for on in legs:
        sol = lib.Solver(prm, N_AGENTS, N_AGENTS)
        dsw = swarm.DeviceSwarm(swarm.SwarmShard(prm, swarm.default_swarm_config(), N_AGENTS, 0, starts, goals), sol)
        if on:
            dsw.set_tracking(sc.gust_model(7, (0.5, 0.0, 0.0), (2.0, 2.0, 1.0), (0.01, 0.01, 0.005)))
        dsw.set_phase_timing(True)
        commit, whole = [], []
        for _ in range(ROUNDS):
            dsw.round()
            ms = dsw.phase_ms()
            commit.append(ms["k_commit"]), whole.append(sum(ms.values()))
        leg = dict(model="on" if on else "off", phase5_ms_median=float(np.median(commit[FIRST:])), round_ms_median=float(np.median(whole[FIRST:])),
                   phase5_ms=[float(x) for x in commit], round_ms=[float(x) for x in whole])
        if on:
            leg["track_stats"] = dsw.track_stats()
            leg["tracking_summary"] = swarm.tracking_summary(dsw.track_records())
        _, _, status, failed = dsw.download(states=False)
        leg["no_solution_so_far"] = int(failed)
        out.append(leg)
        dsw.close(), sol.close()
    return out


def spread(legs, key):
    v = [leg[key] for leg in legs]
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_timing.json"))
    ap.add_argument("--tree", default=None, help="another built checkout: its two 'off' legs are measured in a fresh process")
    ap.add_argument("--alternate", type=int, default=0, help="with --tree: K fresh processes of each checkout, alternated, two 'off' legs each")
    ap.add_argument("--off-only", action="store_true", help="(the child process of --tree) print the 'off' legs of --tree")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)        # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 540)
    if args.off_only:
        print("RESULT " + json.dumps(measure(os.path.abspath(args.tree), (False, False))), flush=True)
        return
    res = dict(method="BASELINE cfg 4's device loop (1024 agents, circle, free space, H = 10) flown from its start with the tracking model off / on / "
                      "off / on in one process, phase timing on; per leg the median over rounds 3-12 of entry [5] of hdsm_dswarm_last_phase_ms "
                      "(k_commit and, with the model on, k_track) and of the seven entries summed",
               expectation="k_track is one more small launch inside entry [5]: a few microseconds on a round of about 148 us; off costs nothing",
               agents=N_AGENTS, n_hor=N_HOR, rounds=ROUNDS, median_over_rounds=[FIRST, ROUNDS - 1])
    res["legs"] = measure(ROOT, (False, True, False, True))
    off, on = [g for g in res["legs"] if g["model"] == "off"], [g for g in res["legs"] if g["model"] == "on"]
    for key in ("phase5_ms_median", "round_ms_median"):
        res[key] = dict(off=float(np.mean([g[key] for g in off])), on=float(np.mean([g[key] for g in on])), off_spread=spread(off, key), on_spread=spread(on, key))
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)

    def off_legs(tree):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only", "--tree", tree], capture_output=True, text=True,
                             timeout=300, check=True).stdout
        return json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])

    if args.tree:
        parent = off_legs(args.tree)
        res["parent"] = dict(legs=parent)
        for key in ("phase5_ms_median", "round_ms_median"):
            p = float(np.mean([g[key] for g in parent]))
            allowed = max(spread(off, key), spread(parent, key))
            res["parent"][key] = dict(off=p, off_spread=spread(parent, key), difference=res[key]["off"] - p, allowed=allowed,
                                      agrees=bool(abs(res[key]["off"] - p) <= allowed))
        print("parent", json.dumps({k: v for k, v in res["parent"].items() if k != "legs"}), flush=True)
        if args.alternate > 0:                           # process against process: every entry the mean of a process's two "off" legs
            alt = dict(this=[], parent=[])
            for _ in range(args.alternate):
                for name, tree in (("this", ROOT), ("parent", args.tree)):
                    legs = off_legs(tree)
                    alt[name].append({key: float(np.mean([g[key] for g in legs])) for key in ("phase5_ms_median", "round_ms_median")})
            res["alternated_processes"] = alt
            for key in ("phase5_ms_median", "round_ms_median"):
                a, b = [x[key] for x in alt["this"]], [x[key] for x in alt["parent"]]
                res["alternated_processes"][key] = dict(this_median=float(np.median(a)), this_range=[min(a), max(a)], parent_median=float(np.median(b)),
                                                        parent_range=[min(b), max(b)])
            print("alternated", json.dumps({k: v for k, v in res["alternated_processes"].items() if k.endswith("_median")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
