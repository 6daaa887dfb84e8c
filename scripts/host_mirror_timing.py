"""Wall time of the host mirror's round (CPU only): hdsm_swarm_prepare_corridor + hdsm_swarm_prepare + hdsm_swarm_commit per round on
the 16-agent forest scene of tests/loop_cases.py, 20 rounds, no solver — the first commit is handed a plan that runs along the
reference, every later one the shift fallback (status HDSM_NO_SOLUTION). One JSON line. HDSM_LIBRARY selects the library, so two
builds can be alternated process by process:  HDSM_LIBRARY=/path/libhdsm.so python scripts/host_mirror_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loop_cases as lc  # noqa: E402
from multi_agent_pkgs_amd import swarm  # noqa: E402

ROUNDS = 20


def main():
    prm, cfg = lc.shape_params(lc.SHAPES[0])
    grid, origin = lc.make_world()
    starts, goals = lc.make_scene(0)
    n, N, P = len(starts), prm.n_hor, prm.poly_hor
    shard = swarm.SwarmShard(prm, cfg, n, 0, starts, goals)
    shard.set_world(grid, origin)
    assert shard.route() == 0
    plans, has = np.zeros((n, N + 1, 9)), np.zeros(n, np.uint8)
    ms = []
    for r in range(ROUNDS):
        t0 = time.perf_counter()
        shard.prepare_corridor()
        inp = shard.prepare(plans, has)
        out = dict(traj=np.zeros((n, N + 1, 9)), ctrl=np.zeros((n, N, 3)), used=np.zeros((n, P), np.uint8), status=np.full(n, 2, np.int32))
        if r == 0:
            out["traj"][:, 0], out["traj"][:, 1:, :6], out["used"][:, 0], out["status"][:] = inp["state"], inp["ref"], 1, 0
        plans, has = shard.commit(out)
        ms.append((time.perf_counter() - t0) * 1e3)
    pos = shard.state()[0]
    print(json.dumps(dict(library=os.environ.get("HDSM_LIBRARY", "default"), rounds=ROUNDS, ms_per_round=float(np.mean(ms)),
                          ms_median_round=float(np.median(ms)), moved_m=float(np.linalg.norm(pos - starts, axis=1).mean()))))


if __name__ == "__main__":
    main()
