"""What a vehicle in the loop (k_vehicle) costs a round of the device-resident loop, on the GPU.

Two flights, each flown once from its start in one process with phase timing on: 1024 agents on the circle in free space (BASELINE cfg
4's device loop, H = 10) and 64 agents on the same circle. Commands are on throughout (the vehicle needs them). After a warm-up the
rounds come in alternated blocks — vehicle off / on with n_sub = 1 / off / on with n_sub = 10 / off / on with n_sub = 100, twice — on
ONE flight, and per block the median over its rounds of entry [5] of hdsm_dswarm_last_phase_ms (k_commit, k_command, and k_vehicle
behind them) and of the seven entries summed. A vehicle steers, so the "on" blocks change the flight the later blocks fly; free
space keeps every round the same kind of round.

EXPECTATION, written down before the run: the cost is one more dependent launch inside entry [5]; it is proportional to
step_plan * n_sub; it is nearly independent of the agent count up to a few thousand, because it is latency (one lane per agent, a
chain of about 20 divisions and 4 derivative evaluations per sub-step), not work; it is of the order of a microsecond per sub-step,
so n_sub = 100 would about double a free-space round (0.11 ms).

--tree DIR flies the same flights with the package of another checkout (the parent commit, built) in fresh processes, every block
"off" and nothing of the feature called, alternated with this build --alternate K times: "off" agrees with the parent when this
build's median of process medians lies inside the range of the parent's processes. --bench K runs `bench.py --gpus 1 --steps 20
--warmup 5` of both checkouts K times each, alternated, into --bench-out.

--report flies the 1024-agent circle for 40 rounds with the audit on and the default vehicle under hold and under along and reports
the tracking figures, sigma_min flown (the audit that exists on the flown history) against promised (the device audit of the
plans), the instances without a solution and the reseated / clamped counts. Report only.

usage: python scripts/gpu_vehicle_timing.py [--out profiles/vehicle_timing.json] [--report] [--tree DIR [--alternate K] [--bench K
       [--bench-out profiles/vehicle_bench_ab.json]]]
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
WARMUP, BLOCK, REPEATS = 6, 8, 2
N_SUBS = (1, 10, 100)
FLIGHTS = dict(free_1024=1024, circle_64=64)


def make(tree, n):
    sys.path.insert(0, tree)
    from multi_agent_pkgs_amd import lib, swarm
    from multi_agent_pkgs_amd import scenarios as sc
    from multi_agent_pkgs_amd.params import agile_params

    prm, cfg = agile_params(10, max_rows_static=18), swarm.default_swarm_config()
    starts, goals = sc.circle_scenario(n)
    sol = lib.Solver(prm, n, n)
    return sol, swarm.DeviceSwarm(swarm.SwarmShard(prm, cfg, n, 0, starts, goals), sol), sc, swarm


def _block(dsw):
    commit, whole = [], []
    for _ in range(BLOCK):
        dsw.round()
        ms = dsw.phase_ms()
        commit.append(ms["k_commit"]), whole.append(sum(ms.values()))
    return dict(phase5_ms_median=float(np.median(commit)), round_ms_median=float(np.median(whole)), phase5_ms=[float(x) for x in commit])


def measure(tree, flight, vehicle):
    """The blocks of one flight: `vehicle` False flies every block off and calls nothing of the feature (any checkout)."""
    sol, dsw, sc, _ = make(tree, FLIGHTS[flight])
    dsw.set_phase_timing(True)
    if vehicle:
        dsw.set_commands(True)
    for _ in range(WARMUP):
        dsw.round()
    blocks = []
    for b in range(2 * len(N_SUBS) * REPEATS):
        n_sub = N_SUBS[(b // 2) % len(N_SUBS)] if vehicle and b % 2 == 1 else 0
        if vehicle:
            dsw.set_vehicle(sc.crazyflie_vehicle(n_sub=n_sub) if n_sub else None)
        blocks.append(dict(_block(dsw), n_sub=n_sub))
    out = dict(blocks=blocks, no_solution_so_far=int(dsw.download(states=False)[3]))
    if vehicle:
        out["vehicle_stats"] = dsw.vehicle_stats()
    for key in ("phase5_ms_median", "round_ms_median"):
        for n_sub in (0,) + (N_SUBS if vehicle else ()):
            v = [blk[key] for blk in blocks if blk["n_sub"] == n_sub]
            out[f"{key}_{'off' if n_sub == 0 else 'n_sub_%d' % n_sub}"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    dsw.close(), sol.close()
    return out


def report(n=1024, rounds=40):
    sol, dsw, sc, swarm = make(ROOT, n)
    dsw.close(), sol.close()
    from multi_agent_pkgs_amd import lib
    out = {}
    for feed, name in ((0, "hold"), (1, "along")):
        sol, dsw, sc, swarm = make(ROOT, n)
        dsw.set_audit(True, 1.0), dsw.set_history(rounds), dsw.set_commands(True)
        dsw.set_vehicle(sc.crazyflie_vehicle(feed=feed))
        promised = []
        for _ in range(rounds):
            dsw.round()
            promised.append(float(np.sqrt(dsw.last_audit_round()["sep2"].min())))
        hist = dsw.history(mirror=False)[0]
        recs = swarm.flown_records(hist, sc.circle_scenario(n)[0])
        ones = np.ones(n, np.uint8)
        prm = dsw.shard.prm
        flown = [float(np.sqrt(lib.flight_audit_batch(recs[r], ones, step_plan=1, first=0, n_local=n, drone_radius=prm.drone_radius,
                                                      drone_z_offset=prm.drone_z_offset)["sep2"].min())) for r in range(recs.shape[0])]
        out[name] = dict(tracking=swarm.tracking_summary(dsw.track_records()), sigma_min_promised=min(promised), sigma_min_flown=min(flown),
                         no_solution=int(dsw.download(states=False)[3]), instances=n * rounds, vehicle_stats=dsw.vehicle_stats())
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


def dump(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vehicle_timing.json"))
    ap.add_argument("--report", action="store_true", help="the 1024-agent circle for 40 rounds with the audit on, hold and along (report only)")
    ap.add_argument("--tree", default=None, help="another built checkout (the parent commit): its 'off' blocks are measured in fresh processes")
    ap.add_argument("--alternate", type=int, default=0, help="with --tree: K fresh processes of each checkout, alternated, every block off")
    ap.add_argument("--bench", type=int, default=0, help="with --tree: K runs of the bench line of each checkout, alternated")
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "vehicle_bench_ab.json"))
    ap.add_argument("--skip-flights", action="store_true", help="only what --tree / --report ask for")
    ap.add_argument("--off-only", default="", help="(a child process) print the all-off blocks of this flight with the package of --tree")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)        # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 1100)
    if args.off_only:
        print("RESULT " + json.dumps(measure(os.path.abspath(args.tree), args.off_only, False)), flush=True)
        return
    res = dict(method=f"per flight one process: commands on, {WARMUP} warm-up rounds, then {2 * len(N_SUBS) * REPEATS} blocks of {BLOCK} phase-timed rounds, "
                      f"vehicle off / on alternated on the one flight with n_sub {N_SUBS} in turn; per block the median of entry [5] of "
                      "hdsm_dswarm_last_phase_ms (k_commit + k_command + k_vehicle) and of the seven entries summed; per kind the median, minimum "
                      "and maximum over its blocks; per_sub_step_us: the slope of entry [5] between n_sub 10 and 100 (step_plan 1)",
               expectation="one more dependent launch inside entry [5]; proportional to step_plan * n_sub; nearly independent of the agent count up to a "
                           "few thousand (latency, not work); of the order of a microsecond per sub-step, so n_sub = 100 about doubles a free-space "
                           "round (0.11 ms)", flights={})
    if not args.skip_flights:
        for flight in FLIGHTS:
            res["flights"][flight] = m = measure(ROOT, flight, True)
            off = {key: m[f"{key}_off"]["median"] for key in ("phase5_ms_median", "round_ms_median")}
            m["cost_ms"] = {f"n_sub_{s}": {key: m[f"{key}_n_sub_{s}"]["median"] - off[key] for key in off} for s in N_SUBS}
            m["per_sub_step_us"] = 1e3 * (m["phase5_ms_median_n_sub_100"]["median"] - m["phase5_ms_median_n_sub_10"]["median"]) / 90.0
            print(flight, json.dumps({k: v for k, v in m.items() if k != "blocks"}), flush=True)
    if args.report:
        res["report_1024_agents_40_rounds"] = report()
        print("report", json.dumps(res["report_1024_agents_40_rounds"]), flush=True)
    if args.tree:
        tree = os.path.abspath(args.tree)
        for flight in FLIGHTS if args.alternate > 0 else ():
            alt = dict(this=[], parent=[])
            for _ in range(args.alternate):
                for name, t in (("this", ROOT), ("parent", tree)):
                    r = child(["--off-only", flight, "--tree", t])
                    alt[name].append({key: r[f"{key}_off"]["median"] for key in ("phase5_ms_median", "round_ms_median")})
            summ = dict(processes=alt)
            for key in ("phase5_ms_median", "round_ms_median"):
                a, b = [x[key] for x in alt["this"]], [x[key] for x in alt["parent"]]
                summ[key] = dict(this_median=float(np.median(a)), this_range=[min(a), max(a)], parent_median=float(np.median(b)), parent_range=[min(b), max(b)],
                                 off_inside_parent_spread=bool(min(b) <= float(np.median(a)) <= max(b)))
            res["flights"].setdefault(flight, {})["off_against_parent"] = summ
            print(flight, "off against parent", json.dumps({k: v for k, v in summ.items() if k != "processes"}), flush=True)
        if args.bench > 0:
            runs = dict(this_build=[], commit_before=[])
            t0 = time.time()
            for _ in range(args.bench):
                for name, t in (("this_build", ROOT), ("commit_before", tree)):
                    runs[name].append(bench_line(t))
                print("bench", json.dumps(runs), f"{time.time() - t0:.0f} s", flush=True)
            dump(args.bench_out, dict(command="bench.py --gpus 1 --steps 20 --warmup 5, alternated process by process", ms_per_step=runs,
                                      median={k: float(np.median(v)) for k, v in runs.items()}, range={k: [min(v), max(v)] for k, v in runs.items()}))
    dump(args.out, res)


if __name__ == "__main__":
    main()
