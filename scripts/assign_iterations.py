"""The auction's iteration counts on the CPU: hdsm_assign_host (csrc/assign_core.h) over every case of tests/assign_cases.py, the three
large cases of the device tests and 1024 coincident agents against a line, with the budget left open (max_iters = 2^31 - 1). Writes
profiles/assign_iterations.json; the default budget a m + b of include/hdsm_swarm.h is chosen from it: at least four times the count of
every group recorded.

    python scripts/assign_iterations.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assign_cases as ac  # noqa: E402
from multi_agent_pkgs_amd.params import AssignSetting  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "assign_iterations.json")
    extra = [("1024 agents on one point against a line", np.tile([3.0, 4.0, 1.5], (1024, 1)), ac.line(1024, 0.7), None, None)]
    rows, need = [], 0.0
    for case in ac.cases() + ac.large_cases() + extra:
        _, _, stats = ac.run(case, setting=AssignSetting(max_iters=2 ** 31 - 1))
        ok = stats[stats["status"] == 0]
        ok = ok[ok["active"] > 0]
        if not len(ok):
            continue
        worst = ok[np.argmax(ok["iters"] / ok["active"])]
        rows.append(dict(case=case[0], groups=int(len(stats)), m=int(worst["active"]), iters=int(worst["iters"]), phases=int(worst["phases"]),
                         bids=int(worst["bids"]), iters_per_m=round(float(worst["iters"]) / int(worst["active"]), 2),
                         m_largest=int(ok["active"].max()), iters_largest=int(ok["iters"].max())))
        for s in ok:
            need = max(need, (4.0 * int(s["iters"]) - ac.BUDGET_B) / int(s["active"]))
    doc = dict(what="iterations of the integer auction per group, host form, budget open; per case the group with the most iterations per bidder",
               budget=dict(a=ac.BUDGET_A, b=ac.BUDGET_B, rule="default max_iters = a m + b >= 4 x the iterations of every group recorded",
                           smallest_a_that_holds=round(need, 2)),
               cases=rows)
    assert need <= ac.BUDGET_A, need
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["budget"]))


if __name__ == "__main__":
    main()
