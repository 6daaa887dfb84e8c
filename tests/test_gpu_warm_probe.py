"""The warm start's probe on the GPU: the recorded ring of tests/golden/warm_probe_ring.npz (tests/test_warm_probe.py replays it
through the CPU execution of the same source) through hdsm_replan_device, one handle per replay so that the warm store is
carried from round to round, on the shapes the batch size selects with the HDSM_DUO_MIN / HDSM_TRI_MIN / HDSM_QUAD_MIN knobs:
`quad` (the bench line's kernel) and `replan30` for H = 10, `duo48` for H = 12. Every status equals the cold-started oracle's,
trajectories agree within 1e-9, objectives within 1e-9 relative."""
import numpy as np
import pytest

from multi_agent_pkgs_amd.params import agile_params
from warm_probe_cases import KEYS, REPLAYS, compare, ring, ring_oracle  # noqa: F401  (fixtures: one oracle pass for the module)

pytestmark = pytest.mark.gpu

SHAPES = {"quad": ("h10", 10, dict(HDSM_DUO_MIN="1", HDSM_TRI_MIN="1", HDSM_QUAD_MIN="1")),
          "replan30": ("h10", 10, dict(HDSM_DUO_MIN="0")),
          "duo48": ("h12", 12, dict(HDSM_DUO_MIN="1"))}


@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    lib.load()
    return lib


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ring_replay_on_the_device_matches_the_oracle(hdsm, ring, ring_oracle, monkeypatch, shape):
    import torch
    name, horizon, env = SHAPES[shape]
    prm = agile_params(horizon, max_rows_static=18, threads_per_instance=256)   # (the recording's parameters)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    sol = hdsm.Solver(prm, 16, 16)
    # the shape these knobs select for 16 workgroups, by the library's own rule (hdsm::pick_shape, exported by the CPU execution;
    # thresholds as hdsm_create settles them: a threshold that is not set follows the one before it, 0 = never)
    from wave_emu import pywave
    duo = int(env.get("HDSM_DUO_MIN", 257))
    tri = int(env.get("HDSM_TRI_MIN", 513 if duo > 0 else 0))
    quad = int(env.get("HDSM_QUAD_MIN", 769 if tri > 0 else 0))
    knobs = dict(n=3 * horizon, threads=256, P=prm.poly_hor, RS=prm.max_rows_static, duo_min=duo, tri_min=tri, quad_min=quad)
    assert pywave.pick_shape(knobs, 16) == shape
    for k_ in env:
        monkeypatch.delenv(k_)
    dev = torch.device("cuda:0")
    N, P = prm.n_hor, prm.poly_hor
    out = dict(traj=torch.zeros((16, N + 1, 9), dtype=torch.float64, device=dev), ctrl=torch.zeros((16, N, 3), dtype=torch.float64, device=dev),
               used=torch.zeros((16, P), dtype=torch.uint8, device=dev), status=torch.zeros(16, dtype=torch.int32, device=dev),
               obj=torch.zeros(16, dtype=torch.float64, device=dev))
    for r, o in zip(ring[name], ring_oracle[name]):
        kinds = dict(agent_id=np.int32, n_poly=np.int32, n_rows=np.int32, has_plan=np.uint8)
        args = [torch.from_numpy(np.ascontiguousarray(r[k], dtype=kinds.get(k, np.float64))).to(dev) for k in KEYS]
        sol.replan_device(*args, out["traj"], out["ctrl"], out["used"], out["status"], out["obj"])
        torch.cuda.synchronize()
        compare({k: v.cpu().numpy() for k, v in out.items()}, o)
    sol.close()


def test_the_abi_word_is_unchanged(hdsm):
    """All this shows: the library reports ABI 1.9 as before. The library has no read or write of a handle's warm store, so that a store
    written before the probe is accepted is shown on the CPU execution (tests/test_warm_probe.py, from a recorded store)."""
    assert hdsm.load().hdsm_version() == 0x10009
