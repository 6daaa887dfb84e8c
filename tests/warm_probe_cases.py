"""The recorded ring of tests/golden/warm_probe_ring.npz for the warm-start probe tests on the CPU and on the GPU: the replays, the
oracle's answers for them, the comparison."""
import os

import numpy as np
import pytest

from multi_agent_pkgs_amd.params import agile_params

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
# (recording, horizon, shape)
REPLAYS = [("h10", 10, "quad"), ("h12", 12, "duo48")]


@pytest.fixture(scope="module")
def ring():
    z = np.load(os.path.join(HERE, "golden", "warm_probe_ring.npz"))
    out = {}
    for name, _, _ in REPLAYS:
        first, last = (int(v) for v in z[name + "_rounds"])
        out[name] = [{k: z["%s_r%d_%s" % (name, i, k)] for k in KEYS} for i in range(last - first)]
    assert sum(len(v) for v in out.values()) <= 12
    out["parent_store"] = (int(z["h10_parent_store_rounds"][0]), z["h10_parent_store"])
    return out


@pytest.fixture(scope="module")
def ring_oracle(ring, oracle):
    """The oracle's answers for every recorded round, computed once."""
    out = {}
    for name, horizon, _ in REPLAYS:
        prm = agile_params(horizon, max_rows_static=18)
        out[name] = [oracle.replan(prm, *[r[k] for k in KEYS], n_threads=8) for r in ring[name]]
    return out


def compare(e, o):
    """Every status the oracle's; trajectories within 1e-9, objectives within 1e-9 relative."""
    assert (e["status"] == o["status"]).all(), (e["status"].tolist(), o["status"].tolist())
    ok = o["status"] != 2
    if ok.any():
        dt = float(np.abs(e["traj"] - o["traj"])[ok].max())
        dj = float((np.abs(e["obj"] - o["obj"])[ok] / np.maximum(1.0, np.abs(o["obj"][ok]))).max())
        print("max |traj - oracle| %.3e, max rel |obj - oracle| %.3e" % (dt, dj))
        assert dt < 1e-9 and dj < 1e-9, (dt, dj)
