"""Formations: the case table and an independent numpy / Python-int restatement of the rule of csrc/assign_core.h (include/hdsm_swarm.h,
"formations") that tests/test_assign.py (host form, host mirror, CPU) and tests/test_gpu_assign.py (k_assign, the device loop) share.
TEST INFRASTRUCTURE, no tests. The restatement shares no source with the library: the cost is numpy's elementwise IEEE arithmetic in
the order the header states, the auction is whole-array integer arithmetic (argmax, lexsort) where the library scans and keeps keys."""
import itertools

import numpy as np

from multi_agent_pkgs_amd import lib
from multi_agent_pkgs_amd.params import AssignSetting

QUANTUM = 0.01
COST_CAP = 2 ** 34
BID_LIMIT = 2 ** 52
BUDGET_A, BUDGET_B = 240, 256       # the default budget of iterations, 240 m + 256 (include/hdsm_swarm.h)
_MIN = -(2 ** 62)


def cost_matrix(P, S, quantum=QUANTUM):
    """c [m][m] int64: agent i at P[i] taking the slot at S[j]."""
    inv_q2 = 1.0 / (quantum * quantum)
    dx, dy, dz = (P[:, None, c] - S[None, :, c] for c in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((dx * dx + dy * dy) + dz * dz) * inv_q2
    return np.where(t >= float(COST_CAP), COST_CAP, np.minimum(t, float(COST_CAP)).astype(np.int64)).astype(np.int64)


def auction(c, max_iters=0, bid_limit=BID_LIMIT):
    """The rule on the integer matrix c [m][m]: dict(status, has [m] (the object of bidder i), price [m], iters, phases, bids)."""
    m = len(c)
    out = dict(status=0, has=np.arange(m), price=np.zeros(m, np.int64), iters=0, phases=0, bids=0)
    if m == 0:
        return out
    a = -c * (m + 1)
    p = np.zeros(m, np.int64)
    budget = int(max_iters) if max_iters > 0 else BUDGET_A * m + BUDGET_B
    eps = max(1, int(c.max()) * (m + 1) // 2)
    while True:
        owner, has = np.full(m, -1), np.full(m, -1)
        un = np.arange(m)
        while un.size:
            if out["iters"] == budget:
                out["status"] = 1
                return out
            out["iters"] += 1
            out["bids"] += int(un.size)
            v = a[un] - p[None, :]
            rows = np.arange(un.size)
            j = v.argmax(axis=1)                       # (the first maximum: the lowest j)
            best = v[rows, j]
            if m > 1:
                v[rows, j] = _MIN
                w = v.max(axis=1)
            else:
                w = best
            bid = p[j] + (best - w) + eps
            if (bid >= bid_limit).any():
                out["status"] = 3
                return out
            order = np.lexsort((un, -bid, j))          # by object, the highest bid first, the lowest bidder first among equals
            jo = j[order]
            first = np.r_[True, jo[1:] != jo[:-1]]
            wj, wi, wb = jo[first], un[order][first], bid[order][first]
            prev = owner[wj]
            has[prev[prev >= 0]] = -1
            owner[wj], has[wi], p[wj] = wi, wj, wb
            un = np.nonzero(has < 0)[0]
        out["phases"] += 1
        if eps == 1:
            break
        eps = max(1, eps // 4)
    out["has"], out["price"] = has, p
    return out


def partition(n, groups):
    gs = [0, n] if groups is None or len(groups) < 2 else [int(x) for x in groups]
    return list(zip(gs[:-1], gs[1:]))


def solve(pos, slots, groups=None, active=None, quantum=QUANTUM, max_iters=0, bid_limit=BID_LIMIT):
    """The whole problem by the restatement: (slot_of int32 [n], price int64 [n], stats lib.ASSIGN_STATS [groups])."""
    pos, slots = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(slots, np.float64).reshape(-1, 3)
    n = len(pos)
    act = np.ones(n, bool) if active is None else np.asarray(active) != 0
    parts = partition(n, groups)
    slot_of, price, stats = np.full(n, -1, np.int32), np.zeros(n, np.int64), np.zeros(len(parts), lib.ASSIGN_STATS)
    for g, (lo, hi) in enumerate(parts):
        idx = lo + np.nonzero(act[lo:hi])[0]
        m = len(idx)
        st = stats[g]
        st["first"], st["count"], st["active"] = lo, hi - lo, m
        if m == 0:
            continue
        if not np.isfinite(pos[idx]).all():
            st["status"] = 2
            slot_of[idx] = idx
            continue
        c = cost_matrix(pos[idx], slots[idx], quantum)
        r = auction(c, max_iters, bid_limit)
        st["status"], st["phases"], st["iters"], st["bids"] = r["status"], r["phases"], r["iters"], r["bids"]
        if r["status"] == 0:
            slot_of[idx], price[idx] = idx[r["has"]], r["price"]
            st["cost"] = int(c[np.arange(m), r["has"]].sum())
        else:
            slot_of[idx] = idx
    return slot_of, price, stats


def brute_force_cost(c):
    """The least sum of c over all permutations (m <= 7)."""
    m = len(c)
    rows = np.arange(m)
    return min(int(c[rows, list(perm)].sum()) for perm in itertools.permutations(range(m)))


def duality_gap(c, has, price):
    """dual - primal of the scaled problem (benefit a = -c (m + 1)), in Python ints, from the returned assignment and prices alone."""
    m = len(c)
    a = -c * (m + 1)
    primal = int(a[np.arange(m), has].sum())
    dual = int(price.sum()) + int((a - price[None, :]).max(axis=1).sum())
    return dual - primal


# ---- the cases: (name, pos [n][3], slots [n][3], groups or None, active or None) ----
def _cloud(rng, m, side=60.0):
    return rng.uniform(0.0, side, (m, 3))


def line(m, pitch=1.0, origin=(0.0, 0.0, 1.5)):
    out = np.tile(np.asarray(origin, np.float64), (m, 1))
    out[:, 0] += pitch * np.arange(m)
    return out


def cases():
    rng = np.random.default_rng(20261021)
    out = []
    for m in (1, 2, 3, 7, 63, 64, 65, 130):
        out.append((f"random cloud, m = {m}", _cloud(rng, m), _cloud(rng, m), None, None))
    out.append(("all agents on one point against a line", np.tile([3.0, 4.0, 1.5], (64, 1)), line(64, 0.7), None, None))
    out.append(("a line against its reverse", line(33), line(33)[::-1].copy(), None, None))
    gx, gy = np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij")
    lattice = np.stack([gx.ravel(), gy.ravel(), np.full(64, 1.5)], axis=1)
    out.append(("an 8 x 8 lattice against itself shifted by one pitch", lattice, lattice + [1.0, 0.0, 0.0], None, None))
    ang = 2.0 * np.pi * np.arange(40) / 40
    circle = np.stack([18.0 + 22.0 * np.cos(ang), 15.0 + 22.0 * np.sin(ang), np.full(40, 1.5)], axis=1)
    out.append(("a circle against its antipodal roll", circle, np.roll(circle, 20, axis=0), None, None))
    out.append(("everything at the origin", np.zeros((17, 3)), np.zeros((17, 3)), None, None))
    out.append(("a partition of 1, 63 and 66", _cloud(rng, 130), _cloud(rng, 130), [0, 1, 64, 130], None))
    out.append(("257 groups of 5", _cloud(rng, 1285, 12.0), _cloud(rng, 1285, 12.0), list(range(0, 1286, 5)), None))
    active = (rng.uniform(size=40) < 0.6).astype(np.uint8)
    active[7:15] = 0                                  # (the second group has no active agent)
    active[0], active[39] = 1, 0
    out.append(("an inactive mask, one group without an active agent", _cloud(rng, 40), _cloud(rng, 40), [0, 7, 15, 29, 40], active))
    pos = _cloud(rng, 18)
    pos[7, 1], pos[16, 2] = np.nan, np.inf
    out.append(("positions that are not finite", pos, _cloud(rng, 18), [0, 6, 12, 15, 18], None))
    out.append(("a cloud 10 km wide", _cloud(rng, 20, 1.0e4), _cloud(rng, 20, 1.0e4), None, None))
    return out


def large_cases():
    """What only the device tests and the record of iteration counts run: capacity and its neighbour, two wavefront counts in one launch."""
    rng = np.random.default_rng(7)
    out = [(f"random cloud, m = {m}", _cloud(rng, m), _cloud(rng, m), None, None) for m in (1023, 1024)]
    out.append(("groups of 64 and 65 in one launch", _cloud(rng, 129), _cloud(rng, 129), [0, 64, 129], None))
    return out


def run(case, setting=None, device=None):
    """lib.assign on a case of the table."""
    _, pos, slots, groups, active = case
    return lib.assign(pos, slots, groups=groups, active=active, setting=setting or AssignSetting(), device=device)
