"""Restatement of the projective ICP's per-pixel weights (the *_weighted_* entry points of gs_picp.hip, gs_picp_color.hip,
gs_picp_scale.hip and gs_picp_bwd.hip) in NumPy, on top of tests/picp_ref.py, picp_robust_ref.py, picp_scale_ref.py,
picp_color_ref.py, picp_color_scale_ref.py and picp_grad_ref.py.  TEST INFRASTRUCTURE ONLY.

The rule, per lattice slot with pixel p and wp = pixel_weights[p] (float32):

    1  depth[p] > 0, else code 1
    6  wp > 0 and wp < +inf, else code 6 ("masked"): zero, negative, NaN and +inf all mask.  A masked slot is not
       associated (row -1, a = b = 0), not an inlier, in no median, has no colour row and contributes +0.0 to every term
    2 .. 5 as in picp_ref
    wt  = wp * h      one float32 product; h the Huber weight of the raw residual b (picp_robust_ref.slot_weights; 1
                      without a threshold); the clip flag comes from the unweighted float32 b
    wtc = wp * wc     the same for the colour residual of the joint solve
    terms: (double)wt * ((double)x * (double)y) (+ (double)wtc * ((double)x_c * (double)y_c)), as in picp_robust_ref
    the count is the number of used slots; with huber_k / color_huber_k the medians are those of the unweighted |b| / |r|
    over the used / coloured slots (masked slots are neither)

Everything else is the unweighted solve's.  Weights of all ones give its bits; a weight of 0 gives the bits of a depth
of 0 at that pixel, the code tables apart.

Backward (float64, or float32 for the yardstick), W = wp h:  A = sum W a a^T,  g = sum W a b, and with e = u . a,
c = xi . a per used slot and iteration

    w_bar[slot] += h e (b - c),   ab = wp h ((b - c) u - e xi),   bb = e wp (h + h' (b - c))

which slots are masked being a constant like the association and the clip flags."""
import collections

import numpy as np

from tests import picp_color_ref as pcr
from tests import picp_color_scale_ref as csr
from tests import picp_grad_ref as gr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr

F = np.float32
o = pr.o
MASKED = 6
Rows = collections.namedtuple("Rows", sr.Rows._fields)                        # weight: the total weight wt
ColorRows = collections.namedtuple("ColorRows", csr.Rows._fields)             # weight, color_weight: wt, wtc
Association = collections.namedtuple("Association", sr.Association._fields + ("wp",))


def lattice(weights, stride):
    """the float32 weights of the lattice slots (ns,)"""
    return np.ascontiguousarray(np.asarray(weights, F)[::stride, ::stride]).reshape(-1)


def masks(wp):
    """bool: the weights that mask their slot (float32 comparisons: zero, negative, NaN, +inf)"""
    wp = np.asarray(wp, F)
    with np.errstate(invalid="ignore"):
        return ~((wp > 0) & (wp < F(np.inf)))


def slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T, stride, dist_th, dot_th):
    """picp_ref.slot_rows under the rule, plus wp (ns,): a slot with depth whose weight masks it has code 6, row -1 and a
    zero row, whatever the association would have said.  weights=None: no weights (wp = 1)."""
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                   dot_th)
    if weights is None:
        return code, row, a, b, np.ones(code.shape, F)
    wp = lattice(weights, stride)
    m = masks(wp) & (code != 1)
    code, row, a, b = code.copy(), row.copy(), a.copy(), b.copy()
    code[m], row[m], a[m], b[m] = MASKED, -1, 0, 0
    return code, row, a, b, wp


def total_weights(wp, h, live):
    """float32 wp * h where `live`, 0 elsewhere (one product)"""
    with np.errstate(invalid="ignore", over="ignore"):
        wt = np.asarray(wp, F) * np.asarray(h, F)
    assert wt.dtype == F
    wt[~live] = 0
    return wt


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T, huber_delta=0.0, huber_k=0.0,
         stride=1, dist_thresh=0.1, angle_thresh=30.0):
    """one weighted linearisation at T: picp_scale_ref.Rows (weight = wt; delta = the threshold the weights were taken
    with: the median rule's with huber_k > 0 and huber_delta its floor, else huber_delta)"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b, wp = slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T,
                                    stride, dist_th, dot_th)
    used = code == 0
    delta = csr.geometric_scale(b, used, huber_k, huber_delta)
    wt = total_weights(wp, rr.slot_weights(b, delta, used), used)
    return Rows(code, row, a, b, pr.reduce_terms(rr.terms(code, a, b, wt)), int(used.sum()), wt, delta)


def association(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T0, huber_delta=0.0,
                huber_k=0.0, stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_scale_ref.association of the weighted solve, plus wp (ns,): the lattice's pixel weights (1 without weights)"""
    T = np.array(T0, F).reshape(4, 4).copy()
    used, rws, poses, codes, clip = [], [], [], [], []
    trace = np.zeros((numiters, 8), F)
    deltas = np.zeros(numiters, F)
    for it in range(numiters):
        r = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T, huber_delta, huber_k,
                 stride, dist_thresh, angle_thresh)
        poses.append(T.copy())
        used.append(r.code == 0)
        rws.append(np.where(r.code == 0, r.row, -1))
        codes.append(r.code)
        clip.append(rr.clipped(r.b, r.delta) & (r.code == 0))
        deltas[it] = r.delta
        xi = np.zeros(6, F)
        if r.count > 0:
            xi = pr.solve_spd6(r.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:] = F(r.count), F(r.sums[27]), xi
    ns = used[0].shape[0]
    wp = np.ones(ns, F) if weights is None else lattice(weights, stride)
    return Association(np.stack(used), np.stack(rws), np.stack(poses), np.stack(codes), T, trace, np.stack(clip), deltas,
                       wp)


def solve(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T0, huber_delta=0.0, huber_k=0.0,
          stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """(pose, trace (numiters, 8), thresholds (numiters,))"""
    a = association(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T0, huber_delta, huber_k,
                    stride, numiters, damp, dist_thresh, angle_thresh)
    return a.pose, a.trace, a.deltas


# ------------------------------------------------------------------------------------------ the joint solve
def color_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, weights, T, weight,
               huber_delta=0.0, huber_k=0.0, color_huber_delta=0.0, color_huber_k=0.0, stride=1, dist_thresh=0.1,
               angle_thresh=30.0):
    """one weighted joint linearisation at T: picp_color_scale_ref.Rows with the total weights"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b, wp = slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T,
                                    stride, dist_th, dot_th)
    used = code == 0
    ac, bc, colored = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight)
    _, r, _ = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, 1.0)
    delta = csr.geometric_scale(b, used, huber_k, huber_delta)
    cdelta = csr.color_scale(r, colored, color_huber_k, color_huber_delta)
    wt = total_weights(wp, rr.slot_weights(b, delta, used), used)
    wtc = total_weights(wp, rr.slot_weights(r, cdelta, colored), colored)
    sums = pr.reduce_terms(rr.terms(code, a, b, wt) + rr.terms(code, ac, bc, wtc))
    return ColorRows(code, row, a, b, ac, bc, colored, sums, int(used.sum()), int(colored.sum()), wt, wtc, r, delta,
                     cdelta)


def color_solve(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, weights, T0, weight,
                huber_delta=0.0, huber_k=0.0, color_huber_delta=0.0, color_huber_k=0.0, stride=1, numiters=10, damp=1e-8,
                dist_thresh=0.1, angle_thresh=30.0):
    """(pose, trace (numiters, 9), deltas (numiters,), cdeltas (numiters,))"""
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 9), F)
    deltas, cdeltas = np.zeros(numiters, F), np.zeros(numiters, F)
    for it in range(numiters):
        q = color_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, weights, T,
                       weight, huber_delta, huber_k, color_huber_delta, color_huber_k, stride, dist_thresh, angle_thresh)
        deltas[it], cdeltas[it] = q.delta, q.cdelta
        xi = np.zeros(6, F)
        if q.count > 0:
            xi = pr.solve_spd6(q.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:8], trace[it, 8] = F(q.count), F(q.sums[27]), xi, F(q.color_count)
    return T, trace, deltas, cdeltas


# ------------------------------------------------------------------------------------------ the iteration, any dtype
def _step(v, P, N, wp, used, rows_, clip, T, delta, damp):
    """picp_robust_ref._step with the pixel weights: None without inliers"""
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
    h = np.ones(idx.size, dt)
    h[k] = dt.type(delta) / np.abs(b[k])
    hd = np.zeros(idx.size, dt)
    hd[k] = -h[k] / b[k]
    w = wp[idx]
    wa = (w * h)[:, None] * a
    Hm = a.T @ wa + dt.type(damp) * np.eye(6, dtype=dt)
    xi = np.linalg.solve(Hm, wa.T @ b).astype(dt)
    return idx, rows_[idx], vs, p, m, s, a, b, w, h, hd, Hm, xi


def forward(v, P, N, wp, assoc, T0, damp=1e-8, dtype=np.float64):
    """(final pose, the pose each iteration linearised at) of the chained weighted iterations in `dtype`; wp (ns,): the
    lattice's pixel weights (those of masked slots are never read); thresholds, clip flags and association frozen"""
    v, P, N, wp = (np.asarray(x, dtype) for x in (v, P, N, wp))
    T = np.asarray(T0, dtype).reshape(4, 4).copy()
    poses = []
    for k in range(assoc.used.shape[0]):
        poses.append(T.copy())
        st = _step(v, P, N, wp, assoc.used[k], assoc.rows[k], assoc.clipped[k], T, np.float64(F(assoc.deltas[k])), damp)
        if st is not None:
            T = gr.se3_exp(st[-1]) @ T
    return T, np.stack(poses)


def adjoint(v, P, N, wp, assoc, T0, T_bar, damp=1e-8, poses=None, dtype=np.float64):
    """(v_bar, P_bar, N_bar, T0_bar, w_bar (ns,)) of the weighted iterations"""
    v, P, N, wp = (np.asarray(x, dtype) for x in (v, P, N, wp))
    if poses is None:
        _, poses = forward(v, P, N, wp, assoc, T0, damp, dtype)
    poses = np.asarray(poses, dtype)
    Tb = np.zeros((4, 4), dtype)
    Tb[:3] = np.asarray(T_bar, dtype)[:3]
    vb, Pb, Nb, wb = np.zeros_like(v), np.zeros_like(P), np.zeros_like(N), np.zeros(v.shape[0], dtype)
    for k in range(assoc.used.shape[0] - 1, -1, -1):
        Tk = poses[k]
        st = _step(v, P, N, wp, assoc.used[k], assoc.rows[k], assoc.clipped[k], Tk, np.float64(F(assoc.deltas[k])), damp)
        if st is None:
            continue                       # T_{k+1} = T_k
        idx, rows_, vs, p, m, s, a, b, w, h, hd, Hm, xi = st
        xib = gr.se3_exp_adjoint(xi, Tb @ Tk.T)
        u = np.linalg.solve(Hm, xib).astype(dtype)
        new = np.zeros((4, 4), dtype)
        new[:3] = (gr.se3_exp(xi).T @ Tb)[:3]
        c, e = a @ xi, a @ u
        wb[idx] += h * e * (b - c)
        ab = (w * h)[:, None] * ((b - c)[:, None] * u[None, :] - e[:, None] * xi[None, :])
        bb = e * w * (h + hd * (b - c))
        wv = ab[:, 3:]
        sb = np.cross(m, wv) - bb[:, None] * m
        np.add.at(Pb, rows_, bb[:, None] * m)
        np.add.at(Nb, rows_, ab[:, :3] + np.cross(wv, s) + bb[:, None] * (p - s))
        vb[idx] += sb @ Tk[:3, :3]
        new[:3, :3] += sb.T @ vs
        new[:3, 3] += sb.sum(0)
        Tb = new
    return vb, Pb, Nb, Tb, wb


def on_image(x, shape, stride):
    """a per-slot array (ns, ...) as an image (H, W, ...), zero off the lattice"""
    x = np.asarray(x)
    full = np.zeros(tuple(shape) + x.shape[1:], x.dtype)
    lat = full[::stride, ::stride]
    lat[...] = x.reshape(lat.shape)
    return full


# ------------------------------------------------------------------------------------------ fixtures
def block_mask(shape, block=rr.BLOCK):
    """weights of 1 with 0 in `block` (picp_robust_ref.BLOCK: the moved block of the 60 x 80 scenes)"""
    w = np.ones(shape, F)
    w[block] = 0
    return w


def zeroed_depth(fx, weights):
    """the fixture with depth 0 where `weights` masks, the frame maps KEPT (the rule reads them behind the depth test)"""
    fx = dict(fx)
    depth = np.array(fx["depth"], F)
    depth[masks(weights)] = 0
    fx["depth"] = depth
    return fx


def random_weights(shape, seed=7, lo=0.25, hi=2.0, patch=None):
    """float32 weights uniform in [lo, hi], 0 in `patch` (a pair of slices) when given"""
    w = np.random.default_rng(seed).uniform(lo, hi, shape).astype(F)
    if patch is not None:
        w[patch] = 0
    return w


def special_weights(shape, seed=11):
    """weights that hold, scattered: 0, -1, NaN, +inf, -0.0, a denormal and powers of two from 2^-20 to 2^20"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -1.0, np.nan, np.inf, -0.0, 1e-40, -np.inf] + [2.0 ** e for e in range(-20, 21, 4)], F)
    assert pool[5] != 0 and pool[5] < np.finfo(F).tiny
    return pool[rng.integers(0, pool.size, shape)]
