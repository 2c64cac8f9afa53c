"""Float64 restatement of the projective ICP's Gauss-Newton iterations with a FROZEN association, and its adjoint, in
NumPy.  TEST INFRASTRUCTURE ONLY: the arbiter of gs_projective_icp_backward_batch_f32 (gs_picp_bwd.hip).

The association -- which lattice slots are used in iteration k and the map row of each -- is a constant of the
differentiation.  It comes from tests/picp_ref.py's float32 solve, which is bit-exact to the kernel (`association`), as
do the float32 poses T_k every iteration linearised at (the kernel's tape).  With it frozen, one iteration is smooth:

    s = R_k v + t_k,  a = [m ; s x m],  b = m . (p - s),  A = sum a a^T,  g = sum a b,
    xi = (A + damp I)^-1 g,  T_{k+1} = exp(xi) T_k          (no inlier: T_{k+1} = T_k)

`forward` chains the iterations in the working precision from T0 (what the finite differences of the CPU test see);
`adjoint` is its reverse mode.  Given `poses`, every step of `adjoint` is evaluated at poses[k] instead of at the chain's
own pose: that is the adjoint the kernel computes (each step at the taped float32 T_k).  dtype=np.float32 evaluates the
SAME code in float32: the yardstick of tests/picp_backward_cases.py."""
import collections

import numpy as np

from tests import picp_ref as pr

Association = collections.namedtuple("Association", ["used", "rows", "poses", "codes", "pose", "trace"])


def association(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, stride=1, numiters=10, damp=1e-8,
                dist_thresh=0.1, angle_thresh=30.0):
    """tests/picp_ref.solve, keeping per iteration the used slots (numiters, ns) bool, their rows (numiters, ns) int64
    (-1 where the slot is not used), the float32 pose the iteration linearised at (numiters, 4, 4) and the codes; plus
    the final pose and the trace (the forward's results)."""
    T = np.array(T0, np.float32).reshape(4, 4).copy()
    used, rows, poses, codes = [], [], [], []
    trace = np.zeros((numiters, 8), np.float32)
    for it in range(numiters):
        r = pr.rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_thresh,
                    angle_thresh)
        poses.append(T.copy())
        used.append(r.code == 0)
        rows.append(np.where(r.code == 0, r.row, -1))
        codes.append(r.code)
        xi = np.zeros(6, np.float32)
        if r.count > 0:
            xi = pr.solve_spd6(r.sums, damp)
            T = pr.mm4(pr.o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:] = np.float32(r.count), np.float32(r.sums[27]), xi
    return Association(np.stack(used), np.stack(rows), np.stack(poses), np.stack(codes), T, trace)


def lattice(vertex, stride):
    return np.ascontiguousarray(np.asarray(vertex)[::stride, ::stride]).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- SE(3), any dtype
def hat(w):
    z = w.dtype.type(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], w.dtype)


def _coeffs(th):
    s, c = np.sin(th), np.cos(th)
    return s, c, s / th, (1 - c) / th ** 2, (th - s) / th ** 3


def se3_exp(xi):
    dt = xi.dtype
    v, w = xi[:3], xi[3:]
    wh = hat(w)
    th = np.sqrt(w @ w)
    I3 = np.eye(3, dtype=dt)
    if np.float32(th) < np.float32(1e-6):
        R = I3 + wh
        V = R.copy()
    else:
        _, _, A, B, C = _coeffs(th)
        wh2 = wh @ wh
        R = I3 + A * wh + B * wh2
        V = I3 + B * wh + C * wh2
    T = np.eye(4, dtype=dt)
    T[:3, :3] = R
    T[:3, 3] = V @ v
    return T


def se3_exp_adjoint(xi, Tbar):
    """d <Tbar, exp(xi)> / d xi"""
    dt = xi.dtype
    v, w = xi[:3], xi[3:]
    Rb, tb = Tbar[:3, :3], Tbar[:3, 3]
    wh = hat(w)
    th = np.sqrt(w @ w)
    small = np.float32(th) < np.float32(1e-6)
    I3 = np.eye(3, dtype=dt)
    if small:
        V = I3 + wh
    else:
        s, c, A, B, C = _coeffs(th)
        wh2 = wh @ wh
        V = I3 + B * wh + C * wh2
    vb = V.T @ tb
    Vb = np.outer(tb, v)
    if small:
        whb = Rb + Vb
    else:
        Ab = np.sum(Rb * wh)
        Bb = np.sum(Rb * wh2) + np.sum(Vb * wh)
        Cb = np.sum(Vb * wh2)
        W2b = B * Rb + C * Vb
        whb = A * Rb + B * Vb + W2b @ wh.T + wh.T @ W2b
        dA = (c * th - s) / th ** 2
        dB = (s * th - 2 * (1 - c)) / th ** 3
        dC = ((1 - c) * th - 3 * (th - s)) / th ** 4
        thb = Ab * dA + Bb * dB + Cb * dC
    wb = np.array([whb[2, 1] - whb[1, 2], whb[0, 2] - whb[2, 0], whb[1, 0] - whb[0, 1]], dt)
    if not small:
        wb = wb + thb * w / th
    return np.concatenate([vb, wb]).astype(dt)


# ---------------------------------------------------------------------------------------------- the iteration
def _step(v, P, N, used, rows, T, damp):
    """one linearisation at T: None without inliers, else everything the step and its adjoint need"""
    idx = np.nonzero(used)[0]
    if idx.size == 0:
        return None
    dt = v.dtype
    R, t = T[:3, :3], T[:3, 3]
    vs, p, m = v[idx], P[rows[idx]], N[rows[idx]]
    s = vs @ R.T + t
    a = np.concatenate([m, np.cross(s, m)], 1)
    b = np.sum(m * (p - s), 1)
    Hm = a.T @ a + dt.type(damp) * np.eye(6, dtype=dt)
    xi = np.linalg.solve(Hm, a.T @ b).astype(dt)
    return idx, rows[idx], vs, p, m, s, a, b, Hm, xi


def forward(v, P, N, assoc, T0, damp=1e-8, dtype=np.float64):
    """(final pose, the pose each iteration linearised at) of the chained iterations in `dtype`; v (ns, 3): the lattice
    vertices"""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    T = np.asarray(T0, dtype).reshape(4, 4).copy()
    poses = []
    for k in range(assoc.used.shape[0]):
        poses.append(T.copy())
        st = _step(v, P, N, assoc.used[k], assoc.rows[k], T, damp)
        if st is not None:
            T = se3_exp(st[-1]) @ T
    return T, np.stack(poses)


def adjoint(v, P, N, assoc, T0, T_bar, damp=1e-8, poses=None, dtype=np.float64):
    """(v_bar (ns, 3), P_bar, N_bar, T0_bar (4, 4): top three rows, a zero bottom row) for the upstream adjoint T_bar of
    the final pose.  poses=None: the adjoint of `forward` (every step at the chain's own pose); poses (numiters, 4, 4):
    every step at poses[k], the kernel's tape."""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    if poses is None:
        _, poses = forward(v, P, N, assoc, T0, damp, dtype)
    poses = np.asarray(poses, dtype)
    Tb = np.zeros((4, 4), dtype)
    Tb[:3] = np.asarray(T_bar, dtype)[:3]
    vb, Pb, Nb = np.zeros_like(v), np.zeros_like(P), np.zeros_like(N)
    for k in range(assoc.used.shape[0] - 1, -1, -1):
        Tk = poses[k]
        st = _step(v, P, N, assoc.used[k], assoc.rows[k], Tk, damp)
        if st is None:
            continue                       # T_{k+1} = T_k
        idx, rows, vs, p, m, s, a, b, Hm, xi = st
        xib = se3_exp_adjoint(xi, Tb @ Tk.T)
        u = np.linalg.solve(Hm, xib).astype(dtype)
        new = np.zeros((4, 4), dtype)
        new[:3] = (se3_exp(xi).T @ Tb)[:3]
        c, e = a @ xi, a @ u
        ab = (b - c)[:, None] * u[None, :] - e[:, None] * xi[None, :]
        w = ab[:, 3:]
        sb = np.cross(m, w) - e[:, None] * m
        np.add.at(Pb, rows, e[:, None] * m)
        np.add.at(Nb, rows, ab[:, :3] + np.cross(w, s) + e[:, None] * (p - s))
        vb[idx] += sb @ Tk[:3, :3]
        new[:3, :3] += sb.T @ vs
        new[:3, 3] += sb.sum(0)
        Tb = new
    return vb, Pb, Nb, Tb
