"""The random swarm snapshots of the fuzz (tests/test_gpu_fuzz.py)."""
import problems
from multi_agent_pkgs_amd.params import make_params

K = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")


def _case(rng, case):
    n_hor = int(rng.choice([6, 8, 10, 10, 10, 12, 15]))
    n_rob = int(rng.choice([9, 16, 25, 36, 49, 64]))
    kw = dict(spacing=float(rng.choice([0.8, 1.0, 1.3, 1.8, 2.5])), narrow=bool(rng.random() < 0.35),
              turn=bool(rng.random() < 0.5), chamfer=bool(rng.random() < 0.3),
              absent_frac=float(rng.choice([0, 0, 0.2])), speed=(0.0, float(rng.choice([3.0, 6.0, 9.0]))))
    rk4 = bool(rng.random() < 0.3)
    drag = tuple(rng.choice([0.0, 0.0, 0.1, 0.3], 3))
    prm = make_params(n_hor=n_hor, rk4=rk4, drag=drag, max_rows_static=18, poly_hor=int(rng.choice([2, 3, 4])))
    return prm, n_rob, kw, problems.swarm_snapshot(prm, n_rob, seed=1000 + case, **kw)
