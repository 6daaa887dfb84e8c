#!/usr/bin/env python3
"""What one replan round of the bench line spends OUTSIDE the solver kernel, from a `rocprofv3 --kernel-trace` run (kernel trace only,
no counters) of the plain bench command with a second window:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o bench -- python bench.py --gpus 1 --steps 20 --warmup 5 --second-window 100 > line.json
    python scripts/round_overhead.py reduce DIR line.json before|after [profiles/round_overhead.json]

Per timed step of each window: the duration of k_plan_prepass, the gap pre-pass -> solver, the duration of the solver kernel, the gap
solver -> the next step's pre-pass, and "step minus solver" = pre-pass + both gaps; mean and p50 over the timed steps (the figures that
reach into the next step: over the pairs of consecutive timed steps; under the tracer the host is slow, so the means carry the steps at
which the queue ran dry — the p50 is the figure of a queue that is kept full). The solver
dispatches of the timed steps are picked by POSITION in the trace, from the launch sequence the bench line reports (as
scripts/summarize_profile.py does): set-up flight, untimed passes, warm-up, K timed steps; then the second window's warm-up and its K
timed steps. The pre-pass of a step is the last k_plan_prepass dispatch that started before its solver did. (The two clocks of a dispatch
are stamped by the command processor: with nothing between two kernels of a queue a gap can come out a fraction of a microsecond negative.)

    python scripts/round_overhead.py floor DIR [profiles/round_overhead.json]

reduces a trace of scripts/ubench/empty_launch (an empty kernel with the pre-pass's grid, launched back to back on one stream) to the
duration of an empty launch: what no pre-pass can go below.

    python scripts/round_overhead.py line before|after line.json [...] [--out profiles/round_overhead.json]

appends the ms_per_step of both windows of plain (untraced) bench lines: the alternations parent / this tree."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "round_overhead.json")


def stat(xs):
    s = sorted(xs)
    n = len(s)
    p50 = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return {"mean_us": round(sum(s) / n / 1e3, 3), "p50_us": round(p50 / 1e3, 3), "min_us": round(s[0] / 1e3, 3), "max_us": round(s[-1] / 1e3, 3)}


def trace_rows(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def last_json_line(path):
    return json.loads([x for x in open(path).read().strip().splitlines() if x.startswith("{")][-1])


def window(solver, pre, lo, hi):
    """solver, pre: (start, end) sorted by start; steps lo..hi-1 of `solver`. What reaches into the next step (the gap behind the solver, step
    minus solver, the step) is taken over the hi - lo - 1 pairs of consecutive timed steps."""
    out = {"prepass": [], "gap_prepass_to_solver": [], "solver": [], "gap_solver_to_next_prepass": [], "step_minus_solver": [], "step": []}
    j = 0

    def pre_of(s0):   # the last pre-pass dispatched before the solver dispatch that starts at s0
        nonlocal j
        while j + 1 < len(pre) and pre[j + 1][0] <= s0:
            j += 1
        return pre[j]

    for i in range(lo, hi):
        s0, s1 = solver[i]
        p0, p1 = pre_of(s0)
        n0, n1 = pre_of(solver[i + 1][0])
        assert (i == 0 or solver[i - 1][0] < p0) and p0 <= s0 < n0, "every timed solver dispatch has a pre-pass of its own in front"
        out["prepass"].append(p1 - p0), out["gap_prepass_to_solver"].append(s0 - p1), out["solver"].append(s1 - s0)
        if i + 1 < hi:   # (behind the last timed step the host synchronises and does other things: not a gap of the round)
            out["gap_solver_to_next_prepass"].append(n0 - s1)
            out["step_minus_solver"].append((p1 - p0) + (s0 - p1) + (n0 - s1)), out["step"].append(n0 - p0)
    return {k: stat(v) for k, v in out.items()}


def load_out(path):
    return json.load(open(path)) if os.path.exists(path) else {
        "what": "scripts/round_overhead.py: per timed step of the bench line (1024 agents, circle, H = 10; windows 165..184 and 100..119) what the queue "
                "spends outside the solver kernel, from a kernel trace of the plain bench command; `before` = the parent commit, `after` = this tree"}


def reduce(trace_dir, line_path, label, out_path):
    line = last_json_line(line_path)
    seq = line["k_replan_launch_sequence"]
    K, W = seq["timed"], seq["warmup"]
    lo = seq["setup_flight"] + seq.get("untimed_pass", 0) + seq["warmup"]
    rows = trace_rows(trace_dir)
    solver = [(a, b) for a, b, n in rows if "k_replan" in n]
    pre = [(a, b) for a, b, n in rows if "k_plan_prepass" in n]
    names = sorted({n[:60] for a, b, n in rows if "k_replan" in n})
    rec = {"bench_line_of_the_traced_run": {"ms_per_step": line["ms_per_step"], "second_window_ms_per_step": (line.get("second_window") or {}).get("ms_per_step")},
           "solver_kernels_in_trace": names, "timed_slice": [lo, lo + K],
           "window_165": window(solver, pre, lo, lo + K)}
    if line.get("second_window"):
        lo2 = lo + K + W   # (one repetition of warm-up + timed, then the second window's own warm-up)
        rec["timed_slice_second_window"] = [lo2, lo2 + K]
        rec["window_100"] = window(solver, pre, lo2, lo2 + K)
    doc = load_out(out_path)
    doc[label] = rec
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


def floor(trace_dir, out_path):
    rows = [(a, b) for a, b, n in trace_rows(trace_dir) if "k_empty" in n]
    rows = rows[len(rows) // 2:]   # (the second half: code object loaded, clocks up)
    rec = {"what": "an empty 256-thread kernel with the pre-pass's grid (177 workgroups), back to back on one stream (scripts/ubench/empty_launch.hip)",
           "launches": len(rows), "duration": stat([b - a for a, b in rows]),
           "gap_to_next": stat([rows[i + 1][0] - rows[i][1] for i in range(len(rows) - 1)])}
    doc = load_out(out_path)
    doc["empty_launch_floor"] = rec
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


def lines(label, paths, out_path):
    doc = load_out(out_path)
    ab = doc.setdefault("bench_lines", {"what": "ms_per_step of plain bench lines (--gpus 1 --steps 20 --warmup 5 --second-window 100), parent and this tree "
                                                "alternated on one box in one session; each list in the order run"})
    for p in paths:
        z = last_json_line(p)
        ab.setdefault(label, []).append({"window_165_ms_per_step": z["ms_per_step"], "window_100_ms_per_step": z["second_window"]["ms_per_step"]})
    json.dump(doc, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 4 and a[0] == "reduce":
        reduce(a[1], a[2], a[3], a[4] if len(a) > 4 else DEFAULT_OUT)
    elif len(a) >= 2 and a[0] == "floor":
        floor(a[1], a[2] if len(a) > 2 else DEFAULT_OUT)
    elif len(a) >= 3 and a[0] == "line":
        out = DEFAULT_OUT
        if "--out" in a:
            out = a[a.index("--out") + 1]
            a = a[:a.index("--out")]
        lines(a[1], a[2:], out)
    else:
        sys.exit(__doc__)
