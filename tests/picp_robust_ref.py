"""Restatement of the projective ICP's Huber weights (the *_robust_* entry points of gs_picp.hip, gs_picp_color.hip and
gs_picp_bwd.hip) in NumPy, on top of tests/picp_ref.py, tests/picp_color_ref.py and tests/picp_grad_ref.py.
TEST INFRASTRUCTURE ONLY.

Forward (float32, one rounding per operation, no FMA; the division is the IEEE float32 division):

    w  = |b| > delta  ? delta / |b|  : 1      b: the point-to-plane residual of a used slot (a NaN is not clipped)
    wc = |r| > cdelta ? cdelta / |r| : 1      r: the colour residual before color_weight is applied
    a threshold of 0 switches its weight off (w = 1)
    terms: (double)w * ((double)x * (double)y): the exact product, then one rounding; the joint solve adds the colour
    product weighted by wc, the sum rounded once

and everything else is the plain solve's.  With every threshold 0 the functions here return the bits of the plain ones.

Backward (float64, or float32 for the yardstick): the weight is differentiated, which slots are clipped (`clipped`, from
the float32 forward) is a constant like the association:

    w = clipped ? delta / |b| : 1,  w' = clipped ? -w / b : 0,  A = sum w a a^T,  g = sum w a b
    ab = w ((b - c) u - e xi),  bb = e (w + w' (b - c)),  and bb takes the place of e in sb, P_bar and N_bar."""
import collections

import numpy as np

from tests import picp_color_ref as pcr
from tests import picp_grad_ref as gr
from tests import picp_ref as pr

F = np.float32
o = pr.o
Rows = collections.namedtuple("Rows", pr.Rows._fields + ("weight",))
ColorRows = collections.namedtuple("ColorRows", pcr.ColorRows._fields + ("weight", "color_weight"))
Association = collections.namedtuple("Association", gr.Association._fields + ("clipped",))


def clipped(r, delta):
    """bool: the residuals the Huber weight clips (float32 comparison; delta == 0: none; NaN: not clipped)"""
    r, delta = np.asarray(r, F), F(delta)
    with np.errstate(invalid="ignore"):
        return (np.abs(r) > delta) & bool(delta > 0)


def slot_weights(r, delta, live=None):
    """float32 weights of the residuals r: delta / |r| where clipped, else 1; 0 where `live` (bool) is False"""
    r = np.asarray(r, F)
    k = clipped(r, delta)
    w = np.ones(r.shape, F)
    w[k] = F(delta) / np.abs(r[k])
    assert w.dtype == F
    if live is not None:
        w[~live] = 0
    return w


def terms(code, a, b, w):
    """(n, 28) float64: the exact products of tests/picp_ref.terms, each multiplied by the slot's weight (one rounding)"""
    return w.astype(np.float64)[:, None] * pr.terms(code, a, b)


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, huber_delta, stride=1, dist_thresh=0.1,
         angle_thresh=30.0):
    """one weighted linearisation at T: picp_ref.Rows with the weighted sums, plus weight (0 where the slot is not used)"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                   dot_th)
    w = slot_weights(b, huber_delta, code == 0)
    return Rows(code, row, a, b, pr.reduce_terms(terms(code, a, b, w)), int((code == 0).sum()), w)


def solve(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_delta, stride=1, numiters=10,
          damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_ref.solve with Huber weights: (pose, trace (numiters, 8) = [count, (float) weighted S[27], xi(6)])"""
    return association(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_delta, stride,
                       numiters, damp, dist_thresh, angle_thresh)[4:6]


def association(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_delta, stride=1,
                numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_grad_ref.association of the weighted solve, plus per iteration the clip flags (numiters, ns) bool from the
    float32 residuals (False where the slot is not used)"""
    T = np.array(T0, F).reshape(4, 4).copy()
    used, rws, poses, codes, clip = [], [], [], [], []
    trace = np.zeros((numiters, 8), F)
    for it in range(numiters):
        r = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, huber_delta, stride, dist_thresh,
                 angle_thresh)
        poses.append(T.copy())
        used.append(r.code == 0)
        rws.append(np.where(r.code == 0, r.row, -1))
        codes.append(r.code)
        clip.append(clipped(r.b, huber_delta) & (r.code == 0))
        xi = np.zeros(6, F)
        if r.count > 0:
            xi = pr.solve_spd6(r.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:] = F(r.count), F(r.sums[27]), xi
    return Association(np.stack(used), np.stack(rws), np.stack(poses), np.stack(codes), T, trace, np.stack(clip))


# ------------------------------------------------------------------------------------------ the colour solve
def color_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight,
               huber_delta, color_huber_delta, stride=1, dist_thresh=0.1, angle_thresh=30.0):
    """one weighted joint linearisation at T"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                   dot_th)
    ac, bc, colored = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight)
    # the colour residual before the weight: 1.0f * r == r
    _, r, _ = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, 1.0)
    w = slot_weights(b, huber_delta, code == 0)
    wc = slot_weights(r, color_huber_delta, colored)
    sums = pr.reduce_terms(terms(code, a, b, w) + terms(code, ac, bc, wc))
    return ColorRows(code, row, a, b, ac, bc, colored, sums, int((code == 0).sum()), int(colored.sum()), w, wc)


def color_solve(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T0, weight,
                huber_delta, color_huber_delta, stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_color_ref.solve with Huber weights: (pose, trace (numiters, 9))"""
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 9), F)
    for it in range(numiters):
        r = color_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight,
                       huber_delta, color_huber_delta, stride, dist_thresh, angle_thresh)
        xi = np.zeros(6, F)
        if r.count > 0:
            xi = pr.solve_spd6(r.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:8], trace[it, 8] = F(r.count), F(r.sums[27]), xi, F(r.color_count)
    return T, trace


# ------------------------------------------------------------------------------------------ the iteration, any dtype
def _step(v, P, N, used, rows_, clip, T, delta, damp):
    """picp_grad_ref._step with the weights of the frozen clip flags: None without inliers"""
    idx = np.nonzero(used)[0]
    if idx.size == 0:
        return None
    dt = v.dtype
    R, t = T[:3, :3], T[:3, 3]
    vs, p, m = v[idx], P[rows_[idx]], N[rows_[idx]]
    s = vs @ R.T + t
    a = np.concatenate([m, np.cross(s, m)], 1)
    b = np.sum(m * (p - s), 1)
    k = clip[idx]
    w = np.ones(idx.size, dt)
    w[k] = dt.type(delta) / np.abs(b[k])
    wd = np.zeros(idx.size, dt)
    wd[k] = -w[k] / b[k]
    wa = w[:, None] * a
    Hm = a.T @ wa + dt.type(damp) * np.eye(6, dtype=dt)
    xi = np.linalg.solve(Hm, wa.T @ b).astype(dt)
    return idx, rows_[idx], vs, p, m, s, a, b, w, wd, Hm, xi


def forward(v, P, N, assoc, T0, delta, damp=1e-8, dtype=np.float64):
    """(final pose, the pose each iteration linearised at) of the chained weighted iterations in `dtype`"""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    T = np.asarray(T0, dtype).reshape(4, 4).copy()
    delta = np.float64(F(delta))
    poses = []
    for k in range(assoc.used.shape[0]):
        poses.append(T.copy())
        st = _step(v, P, N, assoc.used[k], assoc.rows[k], assoc.clipped[k], T, delta, damp)
        if st is not None:
            T = gr.se3_exp(st[-1]) @ T
    return T, np.stack(poses)


def adjoint(v, P, N, assoc, T0, T_bar, delta, damp=1e-8, poses=None, dtype=np.float64):
    """picp_grad_ref.adjoint of the weighted iterations: (v_bar, P_bar, N_bar, T0_bar)"""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    if poses is None:
        _, poses = forward(v, P, N, assoc, T0, delta, damp, dtype)
    poses = np.asarray(poses, dtype)
    delta = np.float64(F(delta))
    Tb = np.zeros((4, 4), dtype)
    Tb[:3] = np.asarray(T_bar, dtype)[:3]
    vb, Pb, Nb = np.zeros_like(v), np.zeros_like(P), np.zeros_like(N)
    for k in range(assoc.used.shape[0] - 1, -1, -1):
        Tk = poses[k]
        st = _step(v, P, N, assoc.used[k], assoc.rows[k], assoc.clipped[k], Tk, delta, damp)
        if st is None:
            continue                       # T_{k+1} = T_k
        idx, rows_, vs, p, m, s, a, b, w, wd, Hm, xi = st
        xib = gr.se3_exp_adjoint(xi, Tb @ Tk.T)
        u = np.linalg.solve(Hm, xib).astype(dtype)
        new = np.zeros((4, 4), dtype)
        new[:3] = (gr.se3_exp(xi).T @ Tb)[:3]
        c, e = a @ xi, a @ u
        ab = w[:, None] * ((b - c)[:, None] * u[None, :] - e[:, None] * xi[None, :])
        bb = e * (w + wd * (b - c))
        wv = ab[:, 3:]
        sb = np.cross(m, wv) - bb[:, None] * m
        np.add.at(Pb, rows_, bb[:, None] * m)
        np.add.at(Nb, rows_, ab[:, :3] + np.cross(wv, s) + bb[:, None] * (p - s))
        vb[idx] += sb @ Tk[:3, :3]
        new[:3, :3] += sb.T @ vs
        new[:3, 3] += sb.sum(0)
        Tb = new
    return vb, Pb, Nb, Tb


# ------------------------------------------------------------------------------------------ the moved-block scene
BLOCK = (slice(15, 38), slice(20, 51))     # 23 x 31 pixels of 60 x 80: 15 % of the image
SHIFT = 0.04                               # metres towards the camera: well inside the 10 cm gate


def moved_block(fx, block=BLOCK):
    """a copy of a fixture (convergence_fixture / textured_fixture; BLOCK is meant for 60 x 80) whose live depth is SHIFT
    nearer in `block`, with the frame maps recomputed from it"""
    fx = dict(fx)
    depth = np.array(fx["depth"])
    blk = depth[block]
    depth[block] = np.where(blk > 0, blk - F(SHIFT), blk)
    v, n, _, _ = o.frame_maps(depth, fx["K"])
    fx["depth"], fx["vertex"], fx["normal"] = depth, v, n
    return fx


def translation_error(T, gt):
    return float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - np.asarray(gt, np.float64)[:3, 3]))
