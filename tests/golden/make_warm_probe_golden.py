"""Writes tests/golden/warm_probe_ring.npz: recorded solver inputs of a ring of 16 agents at 1 m chord (the bench geometry at the
smallest size that still squeezes), flown on the CPU with the oracle as the injected solver (swarm.SwarmLoop). Two recordings:

  h10  H = 10, rounds 9..15: the ring leaves its gridlock, meets again and two agents lose their solution (NV = 32 shapes)
  h12  H = 12, rounds 11..15: the same ring with the longer horizon, for the NV = 48 shapes (n = 36 does not fit NV = 32, and
       n = 30 is refused by the NV = 48 shapes)

  h10_parent_store  the warm store (int32 [16][50], the handle's record format) as the build of the commit BEFORE the probe left
       it after replaying h10's first two rounds on the shape `quad`: what a handle that flew with the old warm start holds.
       Written only with --parent-emu PATH (the libhdsm_wave_emu.so of a checkout of that commit, fda9112); without it the
       array of the existing file is kept.

Arrays only: per round the nine arguments of a level-2 replan. tests/test_warm_probe.py replays them with the warm store carried
over and checks that the recording holds what it is there for (a rejected guess row, a fix-up drop after an accepted row, an
input- or state-box row in a guess). Run from the repository root after __graft_entry__.build():
    python tests/golden/make_warm_probe_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

KEYS = ("agent_id", "state", "ref", "n_poly", "n_rows", "A", "b", "plans", "has_plan")
N_ROB = 16
RECORDINGS = {"h10": (10, 9, 16), "h12": (12, 11, 16)}   # name: (horizon, first round, one past the last round)


def fly(horizon, rounds):
    from multi_agent_pkgs_amd import swarm
    from multi_agent_pkgs_amd.params import agile_params
    from oracle import pyoracle as orc
    prm = agile_params(horizon, max_rows_static=18)
    rec = []

    def solve(inp, plans, has):
        return orc.replan(prm, *[inp[k] for k in KEYS[:7]], plans, has, n_threads=8)

    loop = swarm.SwarmLoop(prm, swarm.default_swarm_config(), N_ROB, solve=solve, radius=0.5 / np.sin(np.pi / N_ROB))
    for _ in range(rounds):
        loop.step(record=rec)
    return rec


def parent_store(out, emu_path):
    """Replays h10's rounds 0 and 1 through another build of the CPU execution, store carried over; returns the store."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from multi_agent_pkgs_amd.params import agile_params
    from wave_emu import pywave
    lib = C.CDLL(os.path.abspath(emu_path))
    lib.wave_last_error.restype = C.c_char_p
    pywave._lib = lib
    prm = agile_params(10, max_rows_static=18)
    store = pywave.new_warm_store(N_ROB)
    for i in range(PARENT_STORE_ROUNDS):
        pywave.replan(prm, *[out["h10_r%d_%s" % (i, k)] for k in KEYS], warm=store, shape="quad")
    return store


PARENT_STORE_ROUNDS = 2


def main():
    out = {}
    for name, (horizon, first, last) in RECORDINGS.items():
        rec = fly(horizon, last)
        for i in range(first, last):
            for k in KEYS:
                out["%s_r%d_%s" % (name, i - first, k)] = rec[i][k]
        out[name + "_rounds"] = np.array([first, last], dtype=np.int32)
    path = os.path.join(HERE, "warm_probe_ring.npz")
    if "--parent-emu" in sys.argv:
        out["h10_parent_store"] = parent_store(out, sys.argv[sys.argv.index("--parent-emu") + 1])
    else:
        out["h10_parent_store"] = np.load(path)["h10_parent_store"]
    out["h10_parent_store_rounds"] = np.array([PARENT_STORE_ROUNDS], dtype=np.int32)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
