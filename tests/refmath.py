"""Independent numpy restatement of the hot path's mathematics, used to CERTIFY oracle and GPU results.

Written separately from oracle/hdsm_oracle.c (different language, different variable ordering, no shared
code): it rebuilds the optimisation problem literally from the reference's model —
variables/bounds/dynamics of Agent::CreateGurobiModel (agent_class.cpp:2071-2167), objective and corridor
rows of Agent::SolveOptimizationProblem (agent_class.cpp:858-1023) — and checks a candidate solution with
solver-independent KKT certificates (stationarity via non-negative least squares on the active rows).
"""
import math

import numpy as np
from scipy.optimize import nnls

ABSENT = 1e20


def step9(prm, x, u):
    """One step of the 9-state model: literal Euler / RK4 of ModelODE (agent_class.cpp:2115-2167)."""
    D = np.array([prm.drag[0], prm.drag[1], prm.drag[2]])

    def f(x):
        return np.concatenate([x[3:6], x[6:9] - D * x[3:6], u])

    dt = prm.dt
    k1 = f(x)
    if not prm.rk4:
        return x + dt * k1
    k2 = f(x + dt / 2 * k1)
    k3 = f(x + dt / 2 * k2)
    k4 = f(x + dt * k3)
    return x + dt * ((k1 + 2 * k2 + 2 * k3 + k4) / 6)


def rollout(prm, state, ctrl):
    N = prm.n_hor
    traj = np.zeros((N + 1, 9))
    traj[0] = state
    for i in range(N):
        traj[i + 1] = step9(prm, traj[i], np.asarray(ctrl[i], dtype=float))
    return traj


def affine_maps(prm, state):
    """traj.flatten() = T0 + T @ ctrl.flatten() with ctrl laid out [N][3] (the ABI layout)."""
    N = prm.n_hor
    T0 = rollout(prm, state, np.zeros((N, 3))).reshape(-1)
    T = np.zeros(((N + 1) * 9, 3 * N))
    zero_state = np.zeros(9)
    base = rollout(prm, zero_state, np.zeros((N, 3))).reshape(-1)
    for k in range(3 * N):
        e = np.zeros(3 * N)
        e[k] = 1.0
        T[:, k] = rollout(prm, zero_state, e.reshape(N, 3)).reshape(-1) - base
    return T0, T


def objective(prm, traj, ctrl, ref):
    """Literal objective (agent_class.cpp:870-883, 2098)."""
    N = prm.n_hor
    J = prm.r_u * float(np.sum(np.asarray(ctrl) ** 2))
    for i in range(1, N + 1):
        w = prm.r_n if i == N else prm.r_x
        for k in range(6):
            J += w[k] * (traj[i][k] - ref[i - 1][k]) ** 2
    return J


def quad_form(prm, state, ref):
    """J(u) = 1/2 u'Hu + g'u + f0 in the ABI's ctrl ordering."""
    N = prm.n_hor
    T0, T = affine_maps(prm, state)
    n = 3 * N
    H = 2 * prm.r_u * np.eye(n)
    g = np.zeros(n)
    f0 = 0.0
    for i in range(1, N + 1):
        w = prm.r_n if i == N else prm.r_x
        for k in range(6):
            if w[k] == 0:
                continue
            row = T[9 * i + k]
            e0 = T0[9 * i + k] - ref[i - 1][k]
            H += 2 * w[k] * np.outer(row, row)
            g += 2 * w[k] * e0 * row
            f0 += w[k] * e0 * e0
    return H, g, f0, T0, T


def linear_rows(prm, state, planes_by_point, tol_fixed=1e-6):
    """All rows of the model in u-space.

    planes_by_point: dict m -> array [K,4] of rows n.p_m <= c (corridor + neighbour rows that the
    chosen assignment imposes on point m, m = 0..N).
    Returns (Aeq, beq, Ain, bin, fixed_ok).
    """
    N = prm.n_hor
    T0, T = affine_maps(prm, state)
    Aeq, beq, Ain, bin_ = [], [], [], []
    for k in range(3, 9):  # v_N = a_N = 0 (agent_class.cpp:2078-2081)
        Aeq.append(T[9 * N + k])
        beq.append(-T0[9 * N + k])
    n = 3 * N
    for i in range(N):  # input box (agent_class.cpp:2185-2186)
        for ax in range(3):
            e = np.zeros(n)
            e[3 * i + ax] = 1
            if abs(prm.u_ub[ax]) < ABSENT:
                Ain.append(e.copy()), bin_.append(prm.u_ub[ax])
            if abs(prm.u_lb[ax]) < ABSENT:
                Ain.append(-e), bin_.append(-prm.u_lb[ax])
    for i in range(1, N):  # state boxes on x_1..x_{N-1} (agent_class.cpp:2084, 2179-2184)
        for k in range(3, 9):
            if abs(prm.x_ub[k]) < ABSENT:
                Ain.append(T[9 * i + k]), bin_.append(prm.x_ub[k] - T0[9 * i + k])
            if abs(prm.x_lb[k]) < ABSENT:
                Ain.append(-T[9 * i + k]), bin_.append(T0[9 * i + k] - prm.x_lb[k])
    fixed_ok = True
    for m, rows in planes_by_point.items():
        rows = np.asarray(rows, dtype=float).reshape(-1, 4)
        for r in rows:
            a = r[0] * T[9 * m + 0] + r[1] * T[9 * m + 1] + r[2] * T[9 * m + 2]
            c = r[3] - (r[0] * T0[9 * m + 0] + r[1] * T0[9 * m + 1] + r[2] * T0[9 * m + 2])
            if m == 0:
                fixed_ok &= bool(-c <= tol_fixed)
                continue
            Ain.append(a), bin_.append(c)
    return (np.array(Aeq), np.array(beq), np.array(Ain).reshape(-1, n), np.array(bin_), fixed_ok)


def rows_for_assignment(N, polys, assign, common=None):
    """dict point m -> rows [K,4] imposed by assignment (polys[i][j] = (A,b)) plus common rows."""
    out = {m: [] for m in range(N + 1)}
    for i in range(N):
        blocks = []
        if assign is not None and assign[i] is not None and assign[i] >= 0:
            A, b = polys[i][assign[i]]
            blocks.append(np.hstack([np.asarray(A, float).reshape(-1, 3), np.asarray(b, float).reshape(-1, 1)]))
        if common is not None and common[i] is not None and len(common[i]):
            blocks.append(np.asarray(common[i], float).reshape(-1, 4))
        for blk in blocks:
            out[i].append(blk)
            out[i + 1].append(blk)
    return {m: (np.vstack(v) if v else np.zeros((0, 4))) for m, v in out.items()}


def kkt_certificate(H, g, Aeq, beq, Ain, bin_, u, act_tol=1e-7):
    """Solver-independent optimality certificate of a strictly convex QP.

    Returns dict(primal_eq, primal_in, stationarity, n_active). Stationarity is the residual of
        H u + g + Aeq' nu + Aact' lam = 0,  lam >= 0
    minimised over (nu free, lam >= 0) — a non-negative least-squares problem."""
    u = np.asarray(u, float).reshape(-1)
    grad = H @ u + g
    r_eq = float(np.max(np.abs(Aeq @ u - beq))) if len(beq) else 0.0
    slack = bin_ - Ain @ u if len(bin_) else np.zeros(0)
    r_in = float(max(0.0, -slack.min())) if len(slack) else 0.0
    act = np.where(slack <= act_tol)[0] if len(slack) else np.zeros(0, int)
    cols = [Ain[act].T] if len(act) else []
    if len(beq):
        cols += [Aeq.T, -Aeq.T]
    if cols:
        M = np.hstack(cols)
        scale = np.linalg.norm(M, axis=0)
        scale[scale == 0] = 1
        lam, rnorm = nnls(M / scale, -grad, maxiter=20 * M.shape[1] + 200)
        stat = float(rnorm)
    else:
        stat = float(np.linalg.norm(grad))
    return dict(primal_eq=r_eq, primal_in=r_in, stationarity=stat, n_active=int(len(act)),
                grad_norm=float(np.linalg.norm(grad)))


def certify(prm, state, ref, ctrl, planes_by_point, act_tol=1e-7):
    H, g, f0, T0, T = quad_form(prm, state, ref)
    Aeq, beq, Ain, bin_, fixed_ok = linear_rows(prm, state, planes_by_point)
    cert = kkt_certificate(H, g, Aeq, beq, Ain, bin_, np.asarray(ctrl).reshape(-1), act_tol)
    cert["fixed_ok"] = fixed_ok
    u = np.asarray(ctrl).reshape(-1)
    cert["obj"] = float(0.5 * u @ H @ u + g @ u + f0)
    return cert


def tasc_plane_algebraic(prm, c, o):
    """The trig-free form used by the HIP kernel: s = r / sqrt(1 - nz^2 + (r/h)^2 nz^2)."""
    c, o = np.asarray(c, float), np.asarray(o, float)
    d = o - c
    nrm = np.linalg.norm(d)
    if nrm == 0:
        return np.zeros(4)
    nh = d / nrm
    r, h = prm.drone_radius, prm.drone_z_offset
    k = r / h
    s = r / np.sqrt(1 - nh[2] ** 2 + k * k * nh[2] ** 2)
    q = (c + o) / 2 - min(2 * s, nrm) / 2 * nh
    c1 = np.array([nh[1], -nh[0], 0.0])
    c2 = np.array([-nh[2], 0.0, nh[0]])
    nf = prm.plane_perturb * (c1 + c2) + prm.plane_perturb * c2 + nh
    return np.array([nf[0], nf[1], nf[2], nf @ q])


# ---- the map-dependent half of the reference trajectory and the commit bookkeeping, statement by statement from the reference ----
# (AC = multi_agent_planner/src/agent_class.cpp.) Plain Python floats (IEEE double, one rounding per operation, no contraction):
# the same number format as the reference, written from its text and not from csrc/swarm_core.h.


def py_raycast(val, dim, start, end, max_dist):
    """voxel_grid_util::Raycast (raycast.cpp:22-183) statement by statement; val(i,j,k) raw voxel, -1 outside."""
    mod = lambda v, m: math.fmod(math.fmod(v, m) + m, m)

    def intbound(s, ds):
        if ds < 0:
            return intbound(-s, -ds)
        s = mod(s, 1)
        return (1 - s) / ds if ds != 0 else math.inf

    sg = lambda x: 0 if x == 0 else (-1 if x < 0 else 1)
    x, y, z = (int(math.floor(c)) for c in start)
    ex, ey, ez = (int(math.floor(c)) for c in end)
    d = [end[k] - start[k] for k in range(3)]
    st = [sg(ex - x), sg(ey - y), sg(ez - z)]
    tm = [intbound(start[k], d[k]) for k in range(3)]
    td = [(st[k] / d[k]) if d[k] != 0 else math.nan for k in range(3)]
    out, hit = [], None
    if st == [0, 0, 0]:
        return [list(end), list(start)], None
    tmax = 0.0
    inside = lambda i, j, k: 0 <= i < dim[0] and 0 <= j < dim[1] and 0 <= k < dim[2]
    while True:
        real = [start[k] + min(1.0, tmax) * d[k] for k in range(3)]
        if inside(x, y, z):
            if val(x, y, z) == 100 and tmax <= 1:
                hit = real
                out.append(real)
                break
            out.append(real)
            if (x - start[0]) ** 2 + (y - start[1]) ** 2 + (z - start[2]) ** 2 > max_dist ** 2:
                break
        if tmax >= 1:
            break
        if (tm[0] < tm[1] and st[0] != 0) or st[1] == 0:
            ax = 0 if ((tm[0] < tm[2] and st[0] != 0) or st[2] == 0) else 2
        else:
            ax = 1 if ((tm[1] < tm[2] and st[1] != 0) or st[2] == 0) else 2
        tmax = tm[ax]
        if ax == 0:
            x += st[0]
        elif ax == 1:
            y += st[1]
        else:
            z += st[2]
        tm[ax] += td[ax]
    return out, hit


def velocity_limit(vmin, vmax, sens_pot, sens_dist, occ, dist):
    """Agent::GetVelocityLimit, AC:1805-1817."""
    return vmin + (vmax - vmin) * (1 - (min(max(occ, 0), 100) / 100) ** sens_pot * (1 / math.exp(sens_dist * dist)))


def local_grid_origin(pos, grid_range, vs):
    """environment_builder.cpp:58-67: origin = floor((position - range / 2) / voxel) * voxel."""
    return np.array([math.floor((pos[k] - grid_range[k] / 2) / vs) * vs for k in range(3)])


def window_value(world, worigin, grid_origin, dim, z_min, vs):
    """val(i, j, k) of an agent's local grid cut out of the world [wz][wy][wx]: -1 outside the grid and below the ground,
    0 outside the world, else the world's raw value."""
    off = [int(round((grid_origin[k] - worigin[k]) / vs)) for k in range(3)]
    gk = int(math.ceil((z_min - grid_origin[2]) / vs - 1e-9))
    wz, wy, wx = world.shape

    def val(i, j, k):
        if not (0 <= i < dim[0] and 0 <= j < dim[1] and 0 <= k < dim[2]):
            return -1
        if k < gk:
            return -1
        g = (i + off[0], j + off[1], k + off[2])
        if not (0 <= g[0] < wx and 0 <= g[1] < wy and 0 <= g[2] < wz):
            return 0
        return int(world[g[2], g[1], g[0]])

    return val


def path_velocity_cap(val, dim, grid_origin, vs, pts, vmin, vmax, sens_pot, sens_dist):
    """The voxel term of Agent::ComputePathVelocity (AC:1695-1767) over the polyline pts (world metres, pts[0] = path start):
    segment by segment, the visited voxels of a clear segment (the distance between path_start in WORLD metres and the visited
    point in LOCAL voxel units, times the voxel size, AC:1735), the collision point of the first segment that is not clear
    (distance in voxel units, AC:1755), then stop. Returns (cap, segs): segs[i] = (limit of segment i, collided) for EVERY segment
    of the polyline — the ones behind the first collision too, which the reference never looks at and which do not enter the cap."""
    pts = [np.asarray(p, dtype=np.float64) for p in pts]
    cap, segs, stopped = vmax, [], False
    for i in range(len(pts) - 1):
        a = [float((pts[i][k] - grid_origin[k]) / vs) for k in range(3)]
        b = [float((pts[i + 1][k] - grid_origin[k]) / vs) for k in range(3)]
        md = math.sqrt(sum((a[k] - b[k]) ** 2 for k in range(3)))
        visited, hit = py_raycast(val, dim, a, b, md)
        v = vmax
        if hit is None:
            for pt in visited + [a]:
                o = val(int(pt[0]), int(pt[1]), int(pt[2]))
                o = 100 if o == -1 else o
                v = min(v, velocity_limit(vmin, vmax, sens_pot, sens_dist, o, float(np.linalg.norm(pts[0] - np.array(pt))) * vs))
        else:
            v = min(v, velocity_limit(vmin, vmax, sens_pot, sens_dist, val(int(hit[0]), int(hit[1]), int(hit[2])),
                                      float(np.linalg.norm(np.array(a) - np.array(hit)))))
        segs.append((v, hit is not None))
        if not stopped:
            cap = min(cap, v)
        stopped = stopped or hit is not None   # AC:1765: the loop ends here; what follows is looked at for the caller's statistics only
    return cap, segs


def keep_only_free(pts, val, grid_origin, vs):
    """Agent::KeepOnlyFreeReference (AC:1665-1693) on the positions pts [n][3]: from the first point (after point 0) in an unknown
    (-1) or occupied (100) voxel on, the last free point is repeated. GetVoxelGlobal truncates (p - origin) / voxel.
    Returns (points, stop): stop = index of that first point, n if there is none."""
    pts = np.array(pts, dtype=np.float64)
    for i in range(1, len(pts)):
        c = ((pts[i] - grid_origin) / vs).astype(int)
        if val(int(c[0]), int(c[1]), int(c[2])) in (-1, 100):
            pts[i:] = pts[i - 1]
            return pts, i
    return pts, len(pts)


def reference_velocities(pts, path_vel):
    """The velocity references of AC:1527-1547 on the final reference positions: path_vel * (p_i - p_{i+1}) / dist where the
    two points are more than 1e-2 apart, else 0; the last point repeats the one before it."""
    n = len(pts)
    out = np.zeros((n, 3))
    v = [0.0, 0.0, 0.0]
    for i in range(n - 1):
        dist = math.sqrt(sum((float(pts[i][k]) - float(pts[i + 1][k])) ** 2 for k in range(3)))
        v = [path_vel * (float(pts[i][k]) - float(pts[i + 1][k])) / dist if dist > 1e-2 else 0.0 for k in range(3)]
        out[i] = v
    out[n - 1] = v
    return out


def path_progress(point, path):
    """path_finding_util::GetPathProgress (path_tools.cpp:419-479), the literal walk in steps of 0.01: returns (progress_final,
    proj_dist, d0) — d0 the distance of `point` to path[0], proj_dist the smallest distance over the samples (d0 if no sample is
    strictly closer)."""
    if len(path) <= 1:
        return 1.0, 0.0, 0.0
    p = [float(point[k]) for k in range(3)]
    path = [[float(q[k]) for k in range(3)] for q in path]
    norm = lambda v: math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    curr = list(path[0])
    dist_min = norm([p[k] - curr[k] for k in range(3)])
    d0 = proj_dist = dist_min
    idx, progress, progress_final = 1, 0.0, 0.0
    samp = 0.01
    while idx < len(path):
        nxt = path[idx]
        diff = [nxt[k] - curr[k] for k in range(3)]
        dist_next = norm(diff)
        if dist_next > samp:
            curr = [curr[k] + samp * diff[k] / dist_next for k in range(3)]
            progress = progress + samp
        else:
            curr = list(nxt)
            idx += 1
            progress = progress + dist_next
        d = norm([p[k] - curr[k] for k in range(3)])
        if d < dist_min:
            proj_dist = dist_min = d
            progress_final = progress
    return progress_final, proj_dist, d0


def reference_increment(traj_1, traj_ref, thresh_dist):
    """Agent::CheckReferenceTrajIncrement (AC:569-585): (increment, proj_dist, d0) for traj_curr_[1] and traj_ref_curr_."""
    progress, proj_dist, d0 = path_progress(traj_1, traj_ref)
    return (1 if (progress > 0 and proj_dist < thresh_dist) else 0), proj_dist, d0


def walk_minimum(point, path):
    """The smallest distance between `point` and the samples of the walk of path_progress AFTER the starting point (the quantity
    the increment decision compares with d0 and thresh_dist)."""
    p = [float(point[k]) for k in range(3)]
    path = [[float(q[k]) for k in range(3)] for q in path]
    norm = lambda v: math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    curr, idx, best = list(path[0]), 1, math.inf
    while idx < len(path):
        nxt = path[idx]
        diff = [nxt[k] - curr[k] for k in range(3)]
        dist_next = norm(diff)
        if dist_next > 0.01:
            curr = [curr[k] + 0.01 * diff[k] / dist_next for k in range(3)]
        else:
            curr = list(nxt)
            idx += 1
        best = min(best, norm([p[k] - curr[k] for k in range(3)]))
    return best


def read_back(traj_prev, ctrl_prev, used_prev, traj_new, ctrl_new, used_new, failed):
    """What SolveOptimizationProblem leaves in traj_curr_ / control_curr_ / poly_used_idx_ (AC:955-1019). traj_prev / ctrl_prev:
    the previous plan ([N+1][9], [N][3]) or None when traj_curr_ is empty. A solve that succeeded stores its result; one that
    failed drops the first state and control of the previous plan and duplicates the last ones — nothing changes without a
    previous plan, and poly_used_idx_ stays what it was either way. Returns (traj, ctrl, used), traj None = still empty."""
    if not failed:
        return np.array(traj_new, dtype=np.float64), np.array(ctrl_new, dtype=np.float64), np.array(used_new, dtype=np.uint8)
    if traj_prev is None:
        return None, None, np.array(used_prev, dtype=np.uint8)
    traj, ctrl = [list(r) for r in np.asarray(traj_prev)], [list(r) for r in np.asarray(ctrl_prev)]
    traj.pop(0)                    # AC:1006-1007
    ctrl.pop(0)
    traj.append(list(traj[-1]))    # AC:1010-1013
    ctrl.append(list(ctrl[-1]))
    return np.array(traj, dtype=np.float64), np.array(ctrl, dtype=np.float64), np.array(used_prev, dtype=np.uint8)


# ---- row f1: the reference trajectory of one agent (GenerateReferenceTrajectory AC:1449-1553 on a path that already starts at the
# starting point, SamplePath AC:1591-1663, the neighbour term of ComputePathVelocity AC:1769-1801, GetVelocityLimit AC:1805-1817)
LD = np.longdouble


def reference_row(n_hor, dt, cfg, agent_id, path, n_path, plans, has_plan, vel_cap=None, ranges=None):
    """Row f1 in numpy.longdouble, one instance at a time, every (step, neighbour) pair evaluated, nothing culled.

    Layouts of hdsm_reference: path [n_inst][pmax][3], plans [n_rob][N + 1][9], has_plan [n_rob]; cfg has the six fields of
    hdsm_ref_config. vel_cap (the voxel term, computed elsewhere) starts the minimum, clipped to path_vel_max. ranges (optional,
    [n_inst][2]): the neighbours of instance k are the ids lo <= j < hi only (neighbour groups).
    Returns (ref_full [n_inst][N + 1][6], ref [n_inst][N][6], path_vel [n_inst], info): the three outputs rounded to double, and
    per instance info[k] = dict(walk=[|dist_next - limit| of every comparison of the walk], vel=[|dist - 1e-2| of every
    velocity row], setter=(neighbour, step) of the pair that set path_vel, or None if the cap did).
    A path of one point gives N copies of it (AC:1597-1608), reported as N + 1 rows and path_vel 0, the project's convention."""
    N = int(n_hor)
    n_inst, n_rob = len(agent_id), len(has_plan)
    pos = np.asarray(plans, dtype=np.float64)[:, :, :3].astype(LD)
    has = np.asarray(has_plan).astype(bool)
    vmin, vmax, kd = LD(cfg.path_vel_min), LD(cfg.path_vel_max), LD(cfg.sens_dist)
    dec_step = LD(cfg.path_vel_dec) * LD(dt)
    weight = []
    for i in range(N + 1):                       # AC:1791-1795 and the clamp of AC:1807-1810
        occ = LD(100) * np.power(LD(cfg.sens_other_agents), LD(i))
        occ = min(max(occ, LD(0)), LD(100))
        weight.append(np.power(occ / LD(100), LD(cfg.sens_pot)))
    full = np.zeros((n_inst, N + 1, 6))
    pvs = np.zeros(n_inst)
    info = []
    for k in range(n_inst):
        me, npts = int(agent_id[k]), int(n_path[k])
        pth = np.asarray(path[k], dtype=np.float64).astype(LD)
        pv = vmax if vel_cap is None else min(LD(vel_cap[k]), vmax)
        setter = None
        lo, hi = (0, n_rob) if ranges is None else (max(int(ranges[k][0]), 0), min(int(ranges[k][1]), n_rob))
        if npts >= 2 and 0 <= me < n_rob and has[me]:
            other = np.zeros(n_rob, dtype=bool)
            other[lo:hi] = has[lo:hi]
            other[me] = False
            ids = np.nonzero(other)[0]
            for i in range(N + 1):               # AC:1770: every state of the agent's own plan
                if ids.size == 0:
                    break
                diff = pos[ids, i] - pos[me, i]
                with np.errstate(all="ignore"):
                    dist = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
                    lim = vmin + (vmax - vmin) * (LD(1) - weight[i] * (LD(1) / np.exp(kd * dist)))
                    below = lim < pv             # (false for a NaN: such a pair limits nothing)
                if below.any():
                    w = int(np.argmin(np.where(below, lim, np.inf)))
                    pv, setter = lim[w], (int(ids[w]), i)
        walk, pts = [], []
        if npts < 2:
            pts = [pth[0]] * N
            pv = LD(0)
        else:
            samp = pv * LD(dt)
            cur, limit, at, done = pth[0], samp, 1, 0
            pts.append(cur)
            while done < N:
                step = pth[at] - cur
                dist_next = np.sqrt(step[0] * step[0] + step[1] * step[1] + step[2] * step[2])
                walk.append(float(abs(dist_next - limit)))
                if dist_next > limit:
                    cur = cur + limit * step / dist_next
                    pts.append(cur)
                    done += 1
                    limit = max(LD(0), samp - dec_step)
                else:
                    cur = pth[at]
                    at += 1
                    if at == npts:
                        pts.extend([pth[npts - 1]] * (N - done))
                        break
                    limit = limit - dist_next
        vel_margin, vel = [], np.zeros(3, dtype=LD)
        rows = np.zeros((len(pts), 6), dtype=LD)
        for i, p in enumerate(pts):
            if i + 1 < len(pts):
                back = p - pts[i + 1]
                dist = np.sqrt(back[0] * back[0] + back[1] * back[1] + back[2] * back[2])
                vel_margin.append(float(abs(dist - LD(1e-2))))
                vel = pv * back / dist if dist > LD(1e-2) else np.zeros(3, dtype=LD)
            rows[i, :3], rows[i, 3:] = p, vel if len(pts) > 1 else 0
        full[k, :len(pts)] = rows.astype(np.float64)
        full[k, len(pts):] = full[k, len(pts) - 1]
        pvs[k] = float(pv)
        info.append(dict(walk=walk, vel=vel_margin, setter=setter))
    return full, full[:, :N].copy(), pvs, info
