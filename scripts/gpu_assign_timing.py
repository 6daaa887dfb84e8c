"""What an assignment (k_assign, csrc/assign_kernels.hip) costs on the GPU, and that a flight which never asks for one pays nothing.

kernel    k_assign alone, by HIP events round the launch (hdsm_internal_assign_batch_timed: inputs uploaded once, the launch repeated), in
          fresh processes: per process one untimed launch, then --reps timed ones and their median; per case the median, minimum and
          maximum over --processes processes. Cases: 1 x 1024 random agents in a 60 m cube, 1 x 1024 agents on one point against a
          line, 64 groups of 64, 256 of 16, 1024 of 4 (random, 60 m cube each). Each with its iterations, bids and phases.
scipy     report only: scipy.optimize.linear_sum_assignment on the host over the same integer matrices, group after group (median of three).
bench     --tree DIR --bench K: `bench.py --gpus 1 --steps 20 --warmup 5` of this build and of another built checkout (the parent
          commit), K runs each, alternated process by process: "off is off" when this build's median lies inside the parent's range.

EXPECTATION, written down before the run: nothing is known about these times. The only prior is the iteration counts of the host form
(profiles/assign_iterations.json: about 7 000 iterations for 1024 random agents, 57 000 for 1024 coincident ones) times a few
microseconds per iteration — four barriers and, for every bidder, one wavefront's scan of 1024 objects (SUPPOSED): tens of milliseconds
for 1024 random agents. The coincident case serves 21 million bids, each a scan of 1024 objects by one of sixteen wavefronts of ONE
compute unit: seconds (SUPPOSED). The small groups run one wavefront each and should end in well under a millisecond.

usage: python scripts/gpu_assign_timing.py [--out profiles/assign_timing.json] [--processes 3] [--reps 5] [--tree DIR --bench K]
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
sys.path.insert(0, ROOT)

CASES = ("1x1024_random", "1x1024_coincident", "64x64", "256x16", "1024x4")


def problem(name):
    """(pos, slots, group_start or None) of a case, from a fixed seed"""
    rng = np.random.default_rng(11)
    if name == "1x1024_coincident":
        slots = np.tile([0.0, 0.0, 1.5], (1024, 1))
        slots[:, 0] += 0.7 * np.arange(1024)
        return np.tile([3.0, 4.0, 1.5], (1024, 1)), slots, None
    groups, m = (1, 1024) if name == "1x1024_random" else tuple(int(x) for x in name.split("x"))
    n = groups * m
    return rng.uniform(0.0, 60.0, (n, 3)), rng.uniform(0.0, 60.0, (n, 3)), None if groups == 1 else np.arange(0, n + 1, m, dtype=np.int32)


def one_process(name, reps):
    import ctypes as C

    from multi_agent_pkgs_amd import lib
    L = lib.load()
    fn = L.hdsm_internal_assign_batch_timed
    fn.restype = C.c_int
    pos, slots, gs = problem(name)
    n, ng = len(pos), 0 if gs is None else len(gs) - 1
    slot_of, price, stats = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(max(ng, 1), lib.ASSIGN_STATS)
    ms = np.zeros(reps + 1, np.float32)

    def ptr(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    rc = fn(0, None, n, ng, ptr(gs), ptr(pos), None, ptr(slots), ptr(slot_of), ptr(price), ptr(stats), reps + 1, ptr(ms))
    assert rc == 0, rc
    if name != "1x1024_coincident":                      # (a minute on the host; tests/assign_cases.py has the case at m = 64)
        host = lib.assign(pos, slots, groups=gs)
        assert np.array_equal(host[0], slot_of) and host[2].tobytes() == stats.tobytes()   # (what was timed is the right answer)
    assert sorted(slot_of.tolist()) == list(range(n))
    return dict(first_ms=float(ms[0]), ms=[float(x) for x in ms[1:]], median_ms=float(np.median(ms[1:])), status=sorted(set(stats["status"].tolist())),
                iters_max=int(stats["iters"].max()), iters_sum=int(stats["iters"].sum()), bids=int(stats["bids"].sum()), phases_max=int(stats["phases"].max()))


def scipy_report(name):
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assign_cases as ac
    pos, slots, gs = problem(name)
    mats = [ac.cost_matrix(pos[lo:hi], slots[lo:hi]) for lo, hi in ac.partition(len(pos), gs)]
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for c in mats:
            linear_sum_assignment(c)
        times.append(1e3 * (time.perf_counter() - t0))
    return dict(host_ms=float(np.median(times)), what="linear_sum_assignment over the groups' integer matrices, one after the other; the matrices given")


def child(args_, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_, capture_output=True, text=True, timeout=limit, check=True).stdout
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])


def bench_line(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                         timeout=400, check=True, cwd=tree).stdout
    return float(json.loads(next(ln for ln in reversed(out.splitlines()) if ln.startswith("{")))["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_timing.json"))
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=None, help="another built checkout (the parent commit) for --bench")
    ap.add_argument("--bench", type=int, default=0, help="with --tree: K runs of the bench line of each checkout, alternated")
    ap.add_argument("--parent-first", action="store_true", help="with --bench: the other checkout runs first in every pair")
    ap.add_argument("--skip-kernel", action="store_true", help="only what --tree asks for")
    ap.add_argument("--one", default="", help="(a child process) time this case and print the result")
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, signal.SIG_DFL)            # SIGALRM's default action ends the process: no run outlives its limit
    signal.setitimer(signal.ITIMER_REAL, 1100)
    if args.one:
        print("RESULT " + json.dumps(one_process(args.one, args.reps)), flush=True)
        return
    res = dict(method=f"k_assign between two HIP events, inputs resident; per fresh process one untimed launch and the median of the next ones "
                      f"({args.reps}; 2 for the coincident case); per case the median and range over {args.processes} processes",
               expectation="nothing known beforehand; iterations of the host form times a few microseconds (SUPPOSED): tens of milliseconds for 1024 random "
                           "agents, seconds for 1024 coincident ones (21 million scans on one compute unit), well under a millisecond for the small groups",
               kernel={})
    if os.path.exists(args.out):
        with open(args.out) as f:
            res.update({k: v for k, v in json.load(f).items() if k in ("kernel", "off_against_parent")})
    for name in () if args.skip_kernel else CASES:
        reps = 2 if name == "1x1024_coincident" else args.reps
        procs = [child(["--one", name, "--reps", str(reps)], 300) for _ in range(args.processes)]
        med = [p["median_ms"] for p in procs]
        res["kernel"][name] = dict(median_ms=float(np.median(med)), range_ms=[min(med), max(med)], iters_max=procs[0]["iters_max"],
                                   iters_sum=procs[0]["iters_sum"], bids=procs[0]["bids"], phases_max=procs[0]["phases_max"], status=procs[0]["status"],
                                   us_per_iteration_of_the_longest_group=1e3 * float(np.median(med)) / max(procs[0]["iters_max"], 1),
                                   processes=procs, scipy=scipy_report(name))
        print(name, json.dumps({k: v for k, v in res["kernel"][name].items() if k != "processes"}), flush=True)
    if args.tree and args.bench > 0:
        tree = os.path.abspath(args.tree)
        runs = dict(this_build=[], commit_before=[])
        order = (("this_build", ROOT), ("commit_before", tree))
        for _ in range(args.bench):
            for name, t in order[::-1] if args.parent_first else order:
                runs[name].append(bench_line(t))
            print("bench", json.dumps(runs), flush=True)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        lo, hi = min(runs["commit_before"]), max(runs["commit_before"])
        res["off_against_parent"] = dict(command="bench.py --gpus 1 --steps 20 --warmup 5, alternated process by process", ms_per_step=runs, median=med,
                                         range={k: [min(v), max(v)] for k, v in runs.items()}, off_inside_parent_range=bool(lo <= med["this_build"] <= hi))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
