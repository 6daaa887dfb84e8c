"""Fuzz of the HIP path against the oracle (-m gpu): many random swarm snapshots — horizons 6..15 (both kernel
instantiations), Euler / RK4, drag, 2..4 polyhedra, tight and loose spacing, narrow / turning / chamfered corridors, absent
neighbours — each solved twice on one handle (cold, then warm-started from its own answer) and compared instance by
instance with the oracle. EVERY device answer is verified: up to H = 10 by the oracle's step-ordered search and, where
that runs into its budget, by its second search order (most infeasible step first, orc_replan_ex); beyond H = 10 by the
second order directly (the enumeration in step order needs minutes per instance there). An oracle answer with status
LIMIT is never accepted as a verdict. Every case also goes through the OTHER launch forms the handle would pick for large
batches or deep trees — the kernels that share a CU (reduced staging area, with the rescue pass for instances that overflow
it) and the split launch (hand-over records + item queue) with one- and two-node budgets, items that hand over again — forced here by
the HDSM_* environment knobs."""
import os

import numpy as np
import pytest

from fuzz_cases import K, _case  # noqa: F401  (scripts/gpu_r6_overflow_*.py take them from here)

pytestmark = pytest.mark.gpu

THREADS = 64
N_CASES = int(os.environ.get("HDSM_FUZZ_CASES", "100"))  # (the round's evidence run uses 500: profiles/r04_fuzz.txt)


FORMS = [dict(),                                                              # what the handle picks for the batch by itself
         dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_ORDER_MIN="1", HDSM_BOUNDS_MIN="1"),  # what a large batch gets: shared-CU
                                                                              # kernels, launch order, sphere prefilter
         dict(HDSM_SPLIT="1", HDSM_SPLIT_BUDGET="2"),                         # split launch: hand-over after two nodes, items of pass 2
         dict(HDSM_SPLIT="1", HDSM_SPLIT_BUDGET="1", HDSM_ITEM_BUDGET="2", HDSM_ITEM_MIN="1",   # ... items that hand over again after two
              HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_QUAD_MIN="1")]        # nodes (records chained per instance), four-per-CU kernel in pass 1


def test_fuzz_every_device_answer_is_verified_by_the_oracle(oracle, monkeypatch):
    from multi_agent_pkgs_amd import lib
    rng = np.random.default_rng(12345)
    tot = n15 = reproved = limits = 0
    worst_t = worst_o = 0.0
    for case in range(N_CASES):
        prm, n_rob, kw, sn = _case(rng, case)
        args = [sn[k] for k in K]
        big = prm.copy()
        big.max_nodes, big.max_qp_iters = 500000, 100000000
        if prm.n_hor <= 10:   # the step-ordered search, bounded; where it runs out of budget the other order finishes the proof
            bounded = prm.copy()
            bounded.max_nodes, bounded.max_qp_iters = 100000, 1000000
            o = oracle.replan(bounded, *args, n_threads=THREADS)
            again = np.where(o["status"] == 1)[0]
            if len(again):
                sub = [sn[k][again] if k not in ("plans", "has_plan") else sn[k] for k in K]
                o2 = oracle.replan(big, *sub, n_threads=THREADS, search=1)
                for k in ("traj", "ctrl", "status", "obj"):
                    o[k][again] = o2[k]
                reproved += len(again)
        else:                 # long horizons: the step-ordered enumeration needs minutes per instance, the other order milliseconds
            o = oracle.replan(big, *args, n_threads=THREADS, search=1)
        assert (o["status"] != 1).all(), (case, np.where(o["status"] == 1)[0].tolist())
        for form in FORMS:
            for k_, v_ in form.items():
                monkeypatch.setenv(k_, v_)
            sol = lib.Solver(prm, n_rob, n_rob)   # fresh handle: cold start; the second call exercises the warm start
            for k_ in form:
                monkeypatch.delenv(k_)
            for rep in range(2):
                g = sol.replan(*args)
                tot += n_rob
                n15 += n_rob * (prm.n_hor == 15)
                limits += int((g["status"] == 1).sum())
                assert (g["status"] == o["status"]).all(), (case, form, rep, kw, np.where(g["status"] != o["status"])[0].tolist(),
                                                            g["status"].tolist(), o["status"].tolist())
                ok = o["status"] == 0
                if ok.any():
                    dt = np.abs(g["traj"] - o["traj"])[ok].reshape(ok.sum(), -1).max(1)
                    do = np.abs(g["obj"] - o["obj"])[ok] / np.maximum(1, np.abs(o["obj"][ok]))
                    assert do.max() < 1e-6, (case, form, rep, float(do.max()))
                    # a different but equally good optimum (objective equal to 1e-9) is a tie of the MIQP, not an error
                    tie = (dt > 1e-6) & (do < 1e-9)
                    assert ((dt < 1e-6) | tie).all(), (case, form, rep, np.where(ok)[0][(dt >= 1e-6) & ~tie].tolist(), dt.max())
                    worst_t = max(worst_t, float(dt[~tie].max()) if (~tie).any() else 0.0)
                    worst_o = max(worst_o, float(do.max()))
            sol.close()
    assert limits == 0 and n15 > 0
    print(f"fuzz: {tot} instance-solves in {N_CASES} cases x {len(FORMS)} launch forms ({n15} at H = 15), all verified; {reproved} instances needed the "
          f"oracle's second search order; worst |dtraj| {worst_t:.2e}, worst rel |dobj| {worst_o:.2e}")
