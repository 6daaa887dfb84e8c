"""The enumerated MIQPs of tests/golden/miqp_enum.npz as replan inputs."""
import os

import numpy as np

import problems
from multi_agent_pkgs_amd.params import make_params

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def enum_cases():
    path = os.path.join(GOLD, "miqp_enum.npz")
    g = np.load(path)
    for k in range(int(g["n_cases"])):
        yield k, {key[len(f"e{k}_"):]: g[key] for key in g.files if key.startswith(f"e{k}_")}


def enum_snapshot(c):
    """The replan inputs of an enumerated case in the ABI layouts (one instance: the agent the case was built for)."""
    N, P = int(c["N"]), int(c["P"])
    prm = make_params(n_hor=N, poly_hor=P, max_rows_static=18)
    a = int(c["agent"])
    polys = [(c["polyA"][j], c["polyb"][j]) for j in range(int(c["npoly"]))]
    n_poly, n_rows, A, b = problems.pack_static([polys], P, prm.max_rows_static)
    args = (np.array([a], np.int32), c["state"][None], c["ref"][None], n_poly, n_rows, A, b, c["plans"], c["has_plan"])
    return prm, polys, args
