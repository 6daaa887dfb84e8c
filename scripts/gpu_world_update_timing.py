"""What a map update costs the device-resident loop, on the GPU.

Two worlds: cfg 3's forest (256 agents, horizon 10) and cfg 5's forest-wall-forest (4096 agents on a 64 x 64 lattice, 66 x 66 x 40
local grids, horizon 15). In each, with the raw world resident (hdsm_dswarm_set_raw_world):

  edit     for edit boxes of 1^3, 8^3, 32^3 voxels and a 66 x 66 x 20 local-grid footprint, round the middle of the world: HIP-event
           time of (a) hdsm_dswarm_update_world_raw_device — the box into the raw grid, the region pre-processing, the cache
           invalidation — and of (b) the yardstick, the full-grid hdsm_map_preprocess_device on the same raw world, in the same
           process on the same stream. A block is `reps` calls between two events (one call is too short to time); blocks of (a)
           and (b) alternate after a warm-up of each; per figure the median of the blocks with min and max. The edits write the
           values the raw grid already holds, so the world — and with it the work of every later block — stays the same.
  flight   twin flights from the same start, one taking an 8^3 edit before every round (same stream, box next to an agent that
           changes every round, again the values already there: the flight itself is the twin's), one taking none. Blocks of
           rounds alternate between the two, timed on the host from the first launch to the device's idle: rounds per second,
           median and spread; and the cache hit rate (hits / polyhedra asked for) of both over the timed rounds.

Every step runs under its own time limit (an interval timer whose signal ends the process), and nothing is tried twice.

usage: python scripts/gpu_world_update_timing.py [--steps cfg3,cfg5] [--out profiles/world_update_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_flight_audit_timing import device_swarm, limit, preprocessed  # noqa: E402
from multi_agent_pkgs_amd import lib  # noqa: E402
from multi_agent_pkgs_amd import scenarios as sc  # noqa: E402
from multi_agent_pkgs_amd.params import default_map_config  # noqa: E402

MAP_CFG = dict(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4)
BOXES = {"1x1x1": (1, 1, 1), "8x8x8": (8, 8, 8), "32x32x32": (32, 32, 32), "66x66x20": (66, 66, 20)}


def scene(step):
    """raw world, origin, and a maker of one (loop, dswarm) with the raw world resident; rounds per block."""
    if step == "cfg3":
        raw, origin = sc.forest_for_circle(256, seed=13)
        make = lambda world: device_swarm(10, 256, world, origin)
        return raw, origin, make, 10
    n_y = 64
    starts, goals = sc.lattice_scenario(n_y, n_y)
    raw, origin = sc.forest_wall_forest(int(np.ceil((10 + 2.01 * n_y) / 30)), int(np.ceil((9 + 2.01 * n_y) / 15)), seed=0)
    make = lambda world: device_swarm(15, n_y * n_y, world, origin, starts=starts, goals=goals, tall=True)
    return raw, origin, make, 5


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[float(x) for x in v])


def box_at(raw, centre, bdim):
    """(lo, the raw values there) of a box of bdim (x, y, z) round `centre`, clipped into the world."""
    wz, wy, wx = raw.shape
    bd = [min(bdim[0], wx), min(bdim[1], wy), min(bdim[2], wz)]
    lo = [int(np.clip(centre[k] - bd[k] // 2, 0, (wx, wy, wz)[k] - bd[k])) for k in range(3)]
    return lo, np.ascontiguousarray(raw[lo[2]:lo[2] + bd[2], lo[1]:lo[1] + bd[1], lo[0]:lo[0] + bd[0]])


def measure_edits(dsw, raw, cfg, st, blocks=7):
    import torch
    wz, wy, wx = raw.shape
    d_raw = torch.from_numpy(raw).cuda()[None].contiguous()
    d_out, d_scr = torch.empty_like(d_raw), torch.empty(2 * d_raw.numel(), dtype=torch.uint8, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        a, b = ev(), ev()
        a.record(st)
        for _ in range(reps):
            fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / reps

    full = lambda: lib.map_preprocess_device(cfg, d_raw, d_out, d_scr, stream=st)
    out = {}
    for name, bdim in BOXES.items():
        lo, vals = box_at(raw, (wx // 2, wy // 2, wz // 2), bdim)
        d_vals = torch.from_numpy(vals).cuda()
        edit = lambda: dsw.update_world_raw(d_vals, lo, stream=st)
        wlo, wdim, blo, bd = lib.map_region_extent(cfg, (wx, wy, wz), lo, vals.shape[::-1])
        reps_a, reps_b = 20, 3
        timed(edit, 3), timed(full, 1)                                 # warm-up of both
        a, b = [], []
        for _ in range(blocks):
            a.append(timed(edit, reps_a)), b.append(timed(full, reps_b))
        out[name] = dict(box=[int(x) for x in vals.shape[::-1]], write_voxels=int(np.prod(wdim)), work_voxels=int(np.prod(bd)),
                         region_plus_invalidation_ms=stat(a), full_grid_ms=stat(b), calls_per_block=[reps_a, reps_b])
    assert np.array_equal(dsw.download_world(), d_out[0].cpu().numpy())  # (the edits changed nothing, and region == full here too)
    return out


def measure_flight(make, raw, origin, cfg, rounds, alternations=5):
    import torch
    world = preprocessed(raw)
    (loop_a, a), (loop_b, b) = make(world), make(world)
    a.set_raw_world(cfg, raw), b.set_raw_world(cfg, raw)
    st = torch.cuda.Stream()
    n = loop_a.n_rob
    turn = [0]

    def fly(dsw, edit):
        edits = []
        if edit:  # (the boxes are on the device before the clock starts: the device form is for values that are made there)
            dsw.download(states=True)
            pos = loop_a.shard.state()[0]
            for _ in range(rounds):
                k = turn[0] % n
                turn[0] += 7
                lo, vals = box_at(raw, np.floor((pos[k] - origin) / 0.3).astype(int) + [4, 0, 0], (8, 8, 8))
                edits.append((torch.from_numpy(vals).cuda(), lo))
        dsw.path_stats()                                               # (synchronises: the block starts on an idle device)
        t0 = time.perf_counter()
        for r in range(rounds):
            if edit:
                dsw.update_world_raw(edits[r][0], edits[r][1], stream=st)
            dsw.round(stream=st)
        dsw.path_stats()
        return rounds / (time.perf_counter() - t0)

    for _ in range(2):                                                 # warm-up of both, the edit's first launches included
        fly(a, True), fly(b, False)
    ca0, cb0 = a.cache_stats(), b.cache_stats()
    with_edits, without = [], []
    for _ in range(alternations):
        with_edits.append(fly(a, True)), without.append(fly(b, False))
    ca1, cb1 = a.cache_stats(), b.cache_stats()
    rate = lambda c1, c0: (c1["hits_same_grid"] + c1["hits_interior"] - c0["hits_same_grid"] - c0["hits_interior"]) / max(1, c1["asked"] - c0["asked"])
    res = dict(agents=n, rounds_per_block=rounds, alternations=alternations, rounds_per_s_editing_every_round=stat(with_edits),
               rounds_per_s_never_editing=stat(without), cache_hit_rate_editing=rate(ca1, ca0), cache_hit_rate_never=rate(cb1, cb0),
               world_stats=a.world_stats(), failed_editing=a.download(states=False)[3], failed_never=b.download(states=False)[3])
    edits = measure_edits(a, raw, cfg, st)
    a.close(), b.close()
    return res, edits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="cfg3,cfg5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_update_timing.json"))
    args = ap.parse_args()
    cfg = default_map_config(**MAP_CFG)
    res = dict(method="edit: HIP events round blocks of calls on one stream, region + invalidation and the full-grid form alternated after a "
                      "warm-up; flight: host clock over blocks of rounds between two device synchronisations, twin flights alternated")
    for step in args.steps.split(","):
        with limit(500):
            raw, origin, make, rounds = scene(step)
            flight, edits = measure_flight(make, raw, origin, cfg, rounds)
            res[step] = dict(world=[int(x) for x in raw.shape[::-1]], flight=flight, edit=edits)
        print(step, json.dumps({"flight": {k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in flight.items()},
                                "edit": {k: (v["region_plus_invalidation_ms"]["median"], v["full_grid_ms"]["median"]) for k, v in edits.items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
