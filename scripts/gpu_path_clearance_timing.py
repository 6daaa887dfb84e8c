"""Time the path step of the device-resident loop in clearance mode (k_dmp) next to the plain step (k_path), on the GPU.

Per scenario and mode: hdsm_dswarm_last_path_ms with path period 1, the median of rounds 3-12 from the start of a flight.
  cfg3   cfg 3's forest, 256 agents, 66 x 66 x 20 local grids, horizon 10
  cfg5   cfg 5's forest-wall-forest, 4096 agents on a 64 x 64 lattice, 66 x 66 x 40 local grids, horizon 15 (also at period 2)
  flight cfg 3's forest, 200 rounds per mode: the mean potential (voxel values 1..99, else 0) under the positions flown
The worlds go through the map pre-processing (0.3 m inflation, 1.5 m potential, power 4), so they carry the potential field.
One process; every step runs under its own time limit (an interval timer whose signal ends the process, also inside a native
call), and nothing is tried twice.

usage: python scripts/gpu_path_clearance_timing.py [--steps cfg3,cfg5,flight] [--out profiles/path_clearance_timing.json]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_agent_pkgs_amd import lib, swarm  # noqa: E402
from multi_agent_pkgs_amd import scenarios as sc  # noqa: E402
from multi_agent_pkgs_amd.params import agile_params, agile_ref_config, default_map_config  # noqa: E402

SEARCH_RAD = 1.8  # agent_default_config.yaml:48


class limit:
    """`with limit(s):` — SIGALRM's default action ends the process after s seconds."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)


def preprocessed(raw):
    return lib.map_preprocess(default_map_config(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4),
                              np.ascontiguousarray(raw, np.int8)[None])[0]


def device_swarm(horizon, n_rob, world, origin, clearance, period, starts=None, goals=None, tall=False):
    prm = agile_params(horizon, max_rows_static=18)
    cfg = swarm.default_swarm_config()
    if tall:
        cfg.grid_range[2], cfg.grid_z_min = 12.0, -6.0
    sol = lib.Solver(prm, n_rob, n_rob)
    rcfg = agile_ref_config()

    def solve(inp, plans, has):
        return sol.replan(inp["agent_id"], inp["state"], inp["ref"], inp["n_poly"], inp["n_rows"], inp["A"], inp["b"], plans, has)

    def ref_dev(ids, path, n_path, plans, has, vel_cap=None):
        full, _, pv = sol.reference(rcfg, ids, path, n_path, plans, has, vel_cap=vel_cap)
        return full, pv

    loop = swarm.SwarmLoop(prm, cfg, n_rob, solve=solve, reference=ref_dev, starts=starts, goals=goals)
    assert loop.set_world(world, origin, route=False) in (0, None)
    loop.pmax = 49
    loop.shard.set_path_clearance(clearance)
    loop.shard.set_path_period(period)
    return loop, swarm.DeviceSwarm(loop.shard, sol)


def time_rounds(dsw, rounds=13):
    dsw.set_phase_timing(True)
    ms, corridor = [], []
    for _ in range(rounds):
        dsw.round()
        ms.append(float(dsw.last_path_ms()))
        corridor.append(float(dsw.phase_ms()["k_corridor"]))
    st = dsw.path_stats()
    launched = [m for m in ms[3:13] if m > 0]
    return dict(path_ms_rounds=ms, path_ms_median_rounds_3_12=float(np.median(launched)) if launched else 0.0,
                k_corridor_ms_median_rounds_3_12=float(np.median(corridor[3:13])), planned=int(st["planned"]), failed=int(st["failed"]),
                launches=int(st["launches"]))


def scenario_timing(name, horizon, n_rob, world, origin, periods, **kw):
    out = {}
    for mode, rad in (("plain", 0.0), ("clearance", SEARCH_RAD)):
        for period in periods if mode == "clearance" else periods[:1]:
            key = mode if period == 1 else "%s_period%d" % (mode, period)
            with limit(240):
                t0 = time.perf_counter()
                loop, dsw = device_swarm(horizon, n_rob, world, origin, rad, period, **kw)
                out[key] = time_rounds(dsw)
                out[key]["period"] = period
                dsw.close()
                out[key]["wall_s"] = time.perf_counter() - t0
            print(name, key, json.dumps({k: v for k, v in out[key].items() if k != "path_ms_rounds"}), flush=True)
    return out


def flight_potential(world, origin, n_rob=256, rounds=200):
    out = {}
    for mode, rad in (("plain", 0.0), ("clearance", SEARCH_RAD)):
        with limit(300):
            loop, dsw = device_swarm(10, n_rob, world, origin, rad, 1)
            pot, dists = [], None
            for _ in range(rounds):
                dsw.round()
                dsw.download(states=True)
                pos, dists, nfail = loop.shard.state()
                v = np.floor((pos - origin) / 0.3).astype(int)
                val = world[v[:, 2], v[:, 1], v[:, 0]].astype(int)
                pot.append(np.where((val >= 1) & (val <= 99), val, 0).mean())
            st = dsw.path_stats()
            out[mode] = dict(mean_potential=float(np.mean(pot)), mean_goal_distance_end=float(dists.mean()), solver_failures=int(nfail.sum()),
                             path_failed=int(st["failed"]), planned=int(st["planned"]))
            dsw.close()
        print("flight", mode, json.dumps(out[mode]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="cfg3,cfg5,flight")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_clearance_timing.json"))
    args = ap.parse_args()
    steps = args.steps.split(",")
    res = dict(search_rad=SEARCH_RAD, method="hdsm_dswarm_last_path_ms, path period 1 unless stated, median of rounds 3-12 from the start of a flight")
    if "cfg3" in steps or "flight" in steps:
        with limit(120):
            raw, origin = sc.forest_for_circle(256, seed=13)
            world3 = preprocessed(raw)
    if "cfg3" in steps:
        res["cfg3_forest_256"] = scenario_timing("cfg3", 10, 256, world3, origin, [1])
    if "flight" in steps:
        res["cfg3_flight_200_rounds"] = flight_potential(world3, origin)
    if "cfg5" in steps:
        with limit(240):
            n_y = 64
            starts, goals = sc.lattice_scenario(n_y, n_y)
            raw, origin5 = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
            world5 = preprocessed(raw)
        res["cfg5_fwf_4096"] = scenario_timing("cfg5", 15, n_y * n_y, world5, origin5, [1, 2], starts=starts, goals=goals, tall=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
