"""What the tests of the solver kernel's CPU execution (tests/wave_emu) share: the argument order, the comparison with the oracle,
the mixed batch."""
import numpy as np

import problems

ARG_KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")



def compare(e, o, tol=1e-8):
    assert (e["status"] == o["status"]).all(), (e["status"].tolist(), o["status"].tolist())
    ok = o["status"] != 2
    if ok.any():
        assert np.abs(e["traj"] - o["traj"])[ok].max() < tol
        assert (np.abs(e["obj"] - o["obj"])[ok] / np.maximum(1, np.abs(o["obj"][ok]))).max() < 1e-8


def _mixed_batch(prm, n_rob, seed, every):
    """Instances that narrow, turn, are chamfered, and neighbours without a plan."""
    sn = problems.swarm_snapshot(prm, n_rob, seed, spacing=1.4, narrow=True, turn=True, chamfer=True, absent_frac=0.25)
    idx = np.arange(0, n_rob, every)
    return [sn[k] if k in ("plans", "has_plan") else sn[k][idx] for k in ARG_KEYS]
