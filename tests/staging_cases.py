"""Batches that drive the staging area (Shm::cand) of each shared-CU kernel shape to the edge of its capacity, for the CPU tests of
the device source (test_wave_shapes.py) and the -m gpu tests (test_gpu_abi.py), and the oracle's verdict on them.

Every case was chosen by measurement with the CPU execution of the kernel source (`peak`: the largest count of staged rows a sweep of
the instance reached, counted past the capacity): a NEAR case stages between 90 % of the capacity and one row less, an OVER case has
instances whose sweeps ask for more rows than there are slots. The tests assert those peaks again, so that a change to the solver
that turns a case into an easy one fails loudly instead of quietly testing nothing.

Dense, slow swarms (1 m or 0.7 m spacing, speeds up to 3 m/s) at the staging radius of the product (0.6 m) reach 256, 384 and
720 rows. The 768 rows of the two-per-CU H = 10 kernel are reached in two ways: a wider staging radius (hdsm_params.stage_radius
1.7 m, which fills the area with near rows so that the hot and cold lists meet) and a 0.7 m lattice of 100 agents, in which one
instance has more VIOLATED rows than slots and must carry HDSM_FLAG_STAGING_OVERFLOW."""
import numpy as np

import problems
from multi_agent_pkgs_amd.params import make_params

K = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
FLAG_STAGING_OVERFLOW = 8

# shape (wave_shapes() name) -> capacity, and the batches: (H, n_rob, spacing, stage_radius, instances)
CASES = {
    "quad": dict(cmax=256, near=(10, 64, 1.0, 0.0, [34, 57]), over=(10, 64, 1.0, 0.0, [0, 3, 41])),
    "tri": dict(cmax=384, near=(10, 64, 1.0, 0.0, [24, 11, 48]), over=(10, 64, 1.0, 0.0, [0, 41, 49])),
    "duo": dict(cmax=768, near=(10, 64, 1.0, 1.7, [0, 49]), over=(10, 100, 0.7, 0.0, [96, 0, 50, 70])),
    "duo48": dict(cmax=720, near=(15, 64, 1.0, 0.0, [18]), over=(15, 64, 1.0, 0.0, [0, 41, 58])),
}
SEED = 4242


def batch(spec):
    """(params, argument list) of a case: instances `inst` of the snapshot, all agents' plans as neighbours."""
    n_hor, n_rob, spacing, radius, inst = spec
    prm = make_params(n_hor=n_hor, max_rows_static=18, poly_hor=4, stage_radius=radius)
    sn = problems.swarm_snapshot(prm, n_rob, seed=SEED, spacing=spacing, narrow=False, turn=False, chamfer=False, absent_frac=0,
                                 speed=(0.0, 3.0))
    idx = np.asarray(inst)
    return prm, [sn[k] if k in ("plans", "has_plan") else sn[k][idx] for k in K]


def verdict(oracle, prm, args, n_threads=8):
    """The oracle's answers, never a LIMIT: up to H = 10 its step-ordered search and, where that runs into its budget, the second
    search order (most infeasible step first); beyond H = 10 the second order directly (as test_gpu_fuzz.py does)."""
    big = prm.copy()
    big.max_nodes, big.max_qp_iters = 500000, 100000000
    if prm.n_hor > 10:
        o = oracle.replan(big, *args, n_threads=n_threads, search=1)
    else:
        bounded = prm.copy()
        bounded.max_nodes, bounded.max_qp_iters = 100000, 1000000
        o = oracle.replan(bounded, *args, n_threads=n_threads)
        again = np.where(o["status"] == 1)[0]
        if len(again):
            o2 = oracle.replan(big, *[a if k in ("plans", "has_plan") else a[again] for k, a in zip(K, args)], n_threads=n_threads, search=1)
            for k in ("traj", "ctrl", "status", "obj"):
                o[k][again] = o2[k]
    assert (o["status"] != 1).all(), "the oracle gave no verdict: %r" % o["status"].tolist()
    return o


def exact_or_flagged(st, traj, obj, flags, o, tol):
    """Per instance: the oracle's answer, or HDSM_FLAG_STAGING_OVERFLOW. Never status 0 with another optimum, never NO_SOLUTION
    without the flag where the oracle finds a feasible answer. Returns the mask of flagged instances."""
    flagged = (flags & FLAG_STAGING_OVERFLOW) != 0
    bad = ~flagged & (st != o["status"])
    assert not bad.any(), ("unflagged answers that are not the oracle's", np.where(bad)[0].tolist(), st.tolist(), o["status"].tolist())
    same = ~flagged & (o["status"] == 0)
    if same.any():
        assert np.abs(traj - o["traj"])[same].max() < tol
        assert (np.abs(obj - o["obj"])[same] / np.maximum(1, np.abs(o["obj"][same]))).max() < 1e-8
    return flagged
