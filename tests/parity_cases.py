"""What the GPU parity tests share: the argument order of a replan call, the comparison with the oracle and its tolerances, the
knobs that force each launch shape, and device outputs made stale before a call."""
import numpy as np

TRAJ_TOL = 1e-7
OBJ_RTOL = 1e-6
ARG_KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")



def compare(g, o, polys=None):
    assert (g["status"] == o["status"]).all(), (g["status"].tolist(), o["status"].tolist())
    ok = o["status"] != 2
    if ok.any():
        assert np.abs(g["traj"] - o["traj"])[ok].max() < TRAJ_TOL
        assert np.abs(g["ctrl"] - o["ctrl"])[ok].max() < TRAJ_TOL * 100  # jerks are O(60)
        rel = np.abs(g["obj"] - o["obj"])[ok] / np.maximum(1.0, np.abs(o["obj"][ok]))
        assert rel.max() < OBJ_RTOL


# every launch shape, forced by the execution knobs on an ordinary batch: (H, threads_per_instance, environment)
FORCED_SHAPES = {"replan30_64": (10, 64, {}), "replan30": (10, 256, dict(HDSM_DUO_MIN="0")),
                 "duo": (10, 256, dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="0", HDSM_QUAD_MIN="0")),
                 "tri": (10, 256, dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_QUAD_MIN="0")),
                 "quad": (10, 256, dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_QUAD_MIN="1")),
                 "replan48_64": (15, 64, {}), "replan48": (15, 256, dict(HDSM_DUO_MIN="0")), "duo48": (15, 256, dict(HDSM_DUO_MIN="1"))}


def stale_outputs(n, N, P, dev):
    import torch
    return dict(traj=torch.full((n, N + 1, 9), np.nan, dtype=torch.float64, device=dev), ctrl=torch.full((n, N, 3), np.nan, dtype=torch.float64, device=dev),
                used=torch.zeros((n, P), dtype=torch.uint8, device=dev), status=torch.full((n,), -1, dtype=torch.int32, device=dev),
                obj=torch.full((n,), np.nan, dtype=torch.float64, device=dev))
