"""Worlds and an independent restatement of the path step's clearance mode (csrc/path_core.h, steps 6a-7') for the clearance tests.

The restatement shares no code with the library. Steps 1-6 (grid, goal, nearest free voxels, BFS, descent) are path_cases' pieces;
then, in numpy and plain Python: the cost grid (6a), the tunnel of DMPlanner::setPath (distance_map_planner.cpp:151-226) with a mask
decided by libm's hypot through ctypes (math.hypot is CPython's own routine since 3.8 and need not round the points on the sphere
the same way), the field as a heapq Dijkstra (6c), the descent (6d), the raw path of Agent::GetPath (agent_class.cpp:537-550) and
ShortenDMPPath (path_tools.cpp:250-312) statement by statement, erase included, on the Python Raycast of test_host.py."""
import ctypes
import ctypes.util
import heapq
import math

import numpy as np

import path_cases as pc
from multi_agent_pkgs_amd import scenarios as sc
from multi_agent_pkgs_amd.params import default_map_config

SEARCH_RAD = 1.8     # agent_default_config.yaml:48 dmp_search_rad
MAX_RN = 15          # a row of the tunnel's mask is one 32-bit word
FIELD = 87168        # voxels of the tunnel the device's field holds
MAX_DESCENT = 6144
NB6 = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]


def tunnel_mask(search_rad, res):
    """rn and the offsets of DMPlanner::setPath's mask: `if (std::hypot(std::hypot(nx, ny), nz) > rn) continue`."""
    rn = int(math.ceil(search_rad / res))
    return rn, [(nx, ny, nz) for nx in range(-rn, rn + 1) for ny in range(-rn, rn + 1) for nz in range(-rn, rn + 1)
                if not _libm.hypot(_libm.hypot(float(nx), float(ny)), float(nz)) > rn]


def preprocessed(raw, map_preprocess):
    """The world the planner sees: raw occupancy through the map pre-processing (row f4) with the shipped 0.3 m inflation, 1.5 m
    potential distance and power 4. map_preprocess: oracle.map_preprocess on the CPU, lib.map_preprocess on the GPU."""
    return map_preprocess(default_map_config(voxel_size=0.3, inflation_dist=0.3, potential_dist=1.5, potential_pow=4),
                          np.ascontiguousarray(raw, np.int8)[None])[0]


def worlds(map_preprocess, forest_seed=21, fwf_seed=3, halo_seeds=(40,)):
    """(name, world, origin, sealed, blocks): cfg 3's forest and cfg 5's forest-wall-forest with the potential field of the map
    pre-processing, and path_cases' halo worlds."""
    raw, origin = sc.forest_for_circle(48, seed=forest_seed)
    yield "forest", preprocessed(raw, map_preprocess), origin, (), ()
    fwf, o2 = sc.forest_wall_forest(seed=fwf_seed)
    yield "fwf", preprocessed(fwf, map_preprocess), o2, (), ()
    for s in halo_seeds:
        w, o3, sealed, blocks = pc.halo_world(np.random.default_rng(s))
        yield "halo%d" % s, w, o3, sealed, blocks


def cost_grid(world, off, ldim=pc.LDIM):
    """6a as an int [k][j][i] array (for the voxels step 1 calls free): the world value if it is 1..99, else 0; the x and y side
    faces and voxels outside the world 0."""
    dx, dy, dz = ldim
    wz, wy, wx = world.shape
    I, J, K = np.arange(dx) + off[0], np.arange(dy) + off[1], np.arange(dz) + off[2]
    c = np.zeros((dz, dy, dx), np.int64)
    ki, ji, ii = (np.nonzero((K >= 0) & (K < wz))[0], np.nonzero((J >= 0) & (J < wy))[0], np.nonzero((I >= 0) & (I < wx))[0])
    sub = world[np.ix_(K[ki], J[ji], I[ii])].astype(np.int64)
    c[np.ix_(ki, ji, ii)] = np.where((sub >= 1) & (sub <= 99), sub, 0)
    c[:, :, 0] = c[:, :, dx - 1] = 0
    c[:, 0, :] = c[:, dy - 1, :] = 0
    return c


def prior(world, off, gk, origin, start, goal, vs=pc.VS, ldim=pc.LDIM):
    """Steps 1-6: (status, dict) with the occupancy, sv, gv, G, whether step 4 moved the goal voxel, and the descent's voxel chain
    from sv to gv, both included (the prior path)."""
    if (ldim[0] + 2) * (ldim[1] + 2) * ldim[2] > pc.PLANE_BITS:
        return 4, None
    occ = pc.occupancy(world, off, gk, ldim)
    G = pc.intermediate_goal(goal, origin, ldim, vs)
    vox = lambda p: [int(math.floor((p[k] - origin[k]) / vs)) for k in range(3)]
    sv0, gv0 = vox(start), vox(G)
    sv, gv = pc._nearest_free(occ, sv0), pc._nearest_free(occ, gv0)
    if sv is None or gv is None:
        return 1, None
    level = np.full(occ.shape, -1, np.int64)
    front = np.zeros(occ.shape, bool)
    front[gv[2], gv[1], gv[0]] = True
    seen = occ | front
    level[front] = 0
    L = 0
    while level[sv[2], sv[1], sv[0]] < 0:
        nxt = pc._dilate6(front) & ~seen
        if not nxt.any():
            return 2, None
        L += 1
        level[nxt] = L
        seen |= nxt
        front = nxt
    if L + 1 > MAX_DESCENT:
        return 4, None
    dz, dy, dx = occ.shape
    chain, v = [tuple(sv)], list(sv)
    for lv in range(L, 0, -1):
        for d in NB6:
            n = [v[0] + d[0], v[1] + d[1], v[2] + d[2]]
            if 0 <= n[0] < dx and 0 <= n[1] < dy and 0 <= n[2] < dz and level[n[2], n[1], n[0]] == lv - 1:
                v = n
                break
        else:
            raise AssertionError("descent stuck")
        chain.append(tuple(v))
    assert chain[-1] == tuple(gv)
    return 0, dict(occ=occ, sv=tuple(sv), gv=tuple(gv), G=G, moved=gv != gv0, chain=chain)


def tunnel(occ, chain, search_rad, vs):
    """6b: T as a boolean [k][j][i] array, or None when the radius is beyond the library's mask."""
    free = ~occ
    if search_rad < 0:
        return free.copy()
    rn, mask = tunnel_mask(search_rad, vs)
    if rn > MAX_RN:
        return None
    dz, dy, dx = occ.shape
    P = np.array(chain)
    T = np.zeros(occ.shape, bool)
    for n in mask:
        q = P + n
        ok = (q[:, 0] >= 0) & (q[:, 0] < dx) & (q[:, 1] >= 0) & (q[:, 1] < dy) & (q[:, 2] >= 0) & (q[:, 2] < dz)
        q = q[ok]
        T[q[:, 2], q[:, 1], q[:, 0]] = True
    return T & free


def dijkstra(T, c, gv):
    """6c: {voxel: D} on T from the goal voxel: D(gv) = c(gv), a step into v adds 1 + c(v)."""
    dz, dy, dx = T.shape
    D = {gv: int(c[gv[2], gv[1], gv[0]])}
    heap = [(D[gv], gv)]
    done = set()
    while heap:
        d, v = heapq.heappop(heap)
        if v in done:
            continue
        done.add(v)
        for o in NB6:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if not (0 <= u[0] < dx and 0 <= u[1] < dy and 0 <= u[2] < dz) or not T[u[2], u[1], u[0]]:
                continue
            nd = d + 1 + int(c[u[2], u[1], u[0]])
            if nd < D.get(u, 1 << 60):
                D[u] = nd
                heapq.heappush(heap, (nd, u))
    return D


def shorten_dmp_path(pts, origin, vs, val, ldim):
    """ShortenDMPPath (path_tools.cpp:250-312) statement by statement on [(global point)]; val(i, j, k) the grid it sees."""
    from refmath import py_raycast as _py_raycast
    inside = lambda i, j, k: 0 <= i < ldim[0] and 0 <= j < ldim[1] and 0 <= k < ldim[2]

    def get_voxel_int(p):  # GetVoxelInt(Vector3d): truncation, -1 outside
        i, j, k = int(p[0]), int(p[1]), int(p[2])
        return val(i, j, k) if inside(i, j, k) else -1

    path = [(p, [(p[k] - origin[k]) / vs for k in range(3)]) for p in pts]  # (global, local)
    i = 0
    while i < len(path) - 1:
        if get_voxel_int(path[i][1]) <= 0:
            i_start, i_end, j = i, i, i + 1
            while j < len(path):
                line_clear = True
                s, e = path[i_start][1], path[j][1]
                d = [s[k] - e[k] for k in range(3)]
                dist = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                visited, hit = _py_raycast(val, ldim, s, e, dist)
                if hit is not None:
                    line_clear = False
                else:
                    for pt in visited:
                        if get_voxel_int(pt) > 0:
                            line_clear = False
                if get_voxel_int(path[j][1]) <= 0 and line_clear:
                    i_end = j
                    j = j + 1
                else:
                    break
            if i_end > i_start:
                del path[i_start + 1:i_end]
        i = i + 1
    return [p for p, _ in path]


def plan(world, off, gk, origin, start, goal, search_rad=SEARCH_RAD, vs=pc.VS, ldim=pc.LDIM):
    """Steps 1-6 and 6a-7'. Returns (status, [points], cost, n_raw, info); info (status 0 or 3) holds occ, c, T, D, the prior chain,
    the new chain and the raw path."""
    start, goal = [float(x) for x in start], [float(x) for x in goal]
    if world is None:
        return 0, [start, goal], 0, 0, None
    if search_rad >= 0 and int(math.ceil(search_rad / vs)) > MAX_RN:
        return 4, [], -1, 0, None
    st, pr = prior(world, off, gk, origin, start, goal, vs, ldim)
    if st:
        return st, [], -1, 0, None
    occ, sv, gv = pr["occ"], pr["sv"], pr["gv"]
    c = cost_grid(world, off, ldim)
    T = tunnel(occ, pr["chain"], search_rad, vs)
    if int(T.sum()) > FIELD:
        return 4, [], -1, 0, None
    D = dijkstra(T, c, gv)
    dz, dy, dx = occ.shape
    chain, v = [sv], sv
    while v != gv:
        want = D[v] - 1 - int(c[v[2], v[1], v[0]])
        for o in NB6:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if 0 <= u[0] < dx and 0 <= u[1] < dy and 0 <= u[2] < dz and T[u[2], u[1], u[0]] and D.get(u) == want:
                v = u
                break
        else:
            raise AssertionError("descent stuck")
        if len(chain) == MAX_DESCENT:
            return 4, [], -1, 0, None
        chain.append(v)
    centre = lambda v: [origin[k] + (v[k] + 0.5) * vs for k in range(3)]
    raw = [start] + [centre(v) for v in chain] + ([] if pr["moved"] else [pr["G"]])
    val = lambda i, j, k: 100 if occ[k, j, i] else int(c[k, j, i])
    out = shorten_dmp_path(raw, origin, vs, val, ldim)
    info = dict(occ=occ, c=c, T=T, D=D, prior=pr["chain"], chain=chain, raw=raw, val=val)
    if len(out) > pc.PATH_PTS:
        return 3, [], -1, 0, info
    return 0, out, D[sv], len(chain), info
