"""Restatement of the projective ICP's Huber threshold from the residuals' median (the *_scaled_* entry points:
gs_picp_scale.hip in front of the robust kernels of gs_picp.hip / gs_picp_color.hip, the taped thresholds in
gs_picp_bwd.hip) in NumPy, on top of tests/picp_robust_ref.py.  TEST INFRASTRUCTURE ONLY.

Per iteration, at the pose T the iteration linearises at, with b the float32 residuals of the used slots (code 0):

    med   = the LOWER median of |b|: the element of 0-based rank (n - 1) // 2 in ascending order -- an element of the
            set, never an average.  Non-negative floats order like their bit patterns read as uint32; the selection is
            the kernel's: a radix selection over the 32 key bits in passes of 11, 11 and 10 bits (histogram of the
            digit over the keys that share the digits found so far, the bin that holds the rank).
    c     = float32(huber_k) * float32(1.4826)         one float32 product
    delta = c * med (one float32 product); the floor where the product is not above it (a NaN included)
    n == 0: delta = +0.0

Weights and terms are tests/picp_robust_ref.py's with delta for huber_delta (delta == 0: every weight 1, the plain bits).
Backward: the thresholds are constants of the pass, one per iteration, like the clip flags."""
import collections

import numpy as np

from tests import picp_color_ref as pcr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr

F = np.float32
o = pr.o
gr = rr.gr
K_HUBER = 1.345                             # 95 % efficiency on Gaussian residuals
MAD_TO_SIGMA = F(1.4826)
PASSES = ((21, 11), (10, 11), (0, 10))      # (shift, bits) of the three digits, most significant first
Rows = collections.namedtuple("Rows", rr.Rows._fields + ("delta",))
Association = collections.namedtuple("Association", rr.Association._fields + ("deltas",))


def constant(huber_k):
    """c: the float32 product (float)huber_k * 1.4826f"""
    c = F(huber_k) * MAD_TO_SIGMA
    assert c.dtype == F
    return c


def select(keys, rank):
    """the uint32 key of 0-based `rank` in ascending order, by the kernel's three-pass radix selection"""
    keys = np.asarray(keys, np.uint32)
    assert 0 <= rank < keys.size
    prefix, known = np.uint32(0), np.uint32(0)
    for shift, nbits in PASSES:
        digit = np.uint32((1 << nbits) - 1)
        live = keys[(keys & known) == prefix]
        hist = np.bincount(((live >> np.uint32(shift)) & digit).astype(np.int64), minlength=1 << nbits)
        incl = np.cumsum(hist)
        b = int(np.searchsorted(incl, rank, side="right"))      # the first bin whose inclusive count exceeds the rank
        rank -= int(incl[b] - hist[b])
        prefix = np.uint32(prefix | np.uint32(b << shift))
        known = np.uint32(known | np.uint32(int(digit) << shift))
    return prefix


def lower_median_abs(b, used):
    """(the lower median of |b[used]| as float32, n); n == 0: (+0.0, 0)"""
    keys = np.abs(np.asarray(b, F)[np.asarray(used, bool)]).view(np.uint32)
    n = int(keys.size)
    if n == 0:
        return F(0.0), 0
    return np.array([select(keys, (n - 1) // 2)], np.uint32).view(F)[0], n


def scale(b, used, huber_k, floor=0.0):
    """float32 threshold of one linearisation: max(c * lower median |b[used]|, floor), +0.0 without a used slot"""
    med, n = lower_median_abs(b, used)
    if n == 0:
        return F(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = constant(huber_k) * med
        assert d.dtype == F
        return d if d > F(floor) else F(floor)


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, huber_k, floor=0.0, stride=1,
         dist_thresh=0.1, angle_thresh=30.0):
    """one linearisation at T with the threshold derived there: picp_robust_ref.Rows plus delta"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                   dot_th)
    used = code == 0
    delta = scale(b, used, huber_k, floor)
    w = rr.slot_weights(b, delta, used)
    return Rows(code, row, a, b, pr.reduce_terms(rr.terms(code, a, b, w)), int(used.sum()), w, delta)


def association(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_k, floor=0.0, stride=1,
                numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_robust_ref.association of the scaled solve, plus the thresholds (numiters,) float32"""
    T = np.array(T0, F).reshape(4, 4).copy()
    used, rws, poses, codes, clip = [], [], [], [], []
    trace = np.zeros((numiters, 8), F)
    deltas = np.zeros(numiters, F)
    for it in range(numiters):
        r = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, huber_k, floor, stride,
                 dist_thresh, angle_thresh)
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
    return Association(np.stack(used), np.stack(rws), np.stack(poses), np.stack(codes), T, trace, np.stack(clip), deltas)


def solve(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_k, floor=0.0, stride=1,
          numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """(pose, trace (numiters, 8), thresholds (numiters,))"""
    a = association(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, huber_k, floor, stride,
                    numiters, damp, dist_thresh, angle_thresh)
    return a.pose, a.trace, a.deltas


def color_solve(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T0, weight, huber_k,
                floor=0.0, color_huber_delta=0.0, stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """picp_robust_ref.color_solve with the geometric threshold from the median of |b|; the colour threshold is the
    constant it was: (pose, trace (numiters, 9), thresholds (numiters,))"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 9), F)
    deltas = np.zeros(numiters, F)
    for it in range(numiters):
        code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride,
                                       dist_th, dot_th)
        used = code == 0
        ac, bc, colored = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight)
        _, r, _ = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, 1.0)
        deltas[it] = scale(b, used, huber_k, floor)
        w = rr.slot_weights(b, deltas[it], used)
        wc = rr.slot_weights(r, color_huber_delta, colored)
        sums = pr.reduce_terms(rr.terms(code, a, b, w) + rr.terms(code, ac, bc, wc))
        xi = np.zeros(6, F)
        if used.any():
            xi = pr.solve_spd6(sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:8], trace[it, 8] = F(used.sum()), F(sums[27]), xi, F(colored.sum())
    return T, trace, deltas


# ------------------------------------------------------------------------------------------ the iteration, any dtype
def _frozen(assoc, deltas):
    deltas = assoc.deltas if deltas is None else deltas
    return [np.float64(F(d)) for d in deltas]


def forward(v, P, N, assoc, T0, deltas=None, damp=1e-8, dtype=np.float64):
    """(final pose, the pose each iteration linearised at) of the chained weighted iterations in `dtype`, every
    iteration with its own frozen threshold (assoc.deltas), frozen clip flags and frozen association"""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    T = np.asarray(T0, dtype).reshape(4, 4).copy()
    deltas = _frozen(assoc, deltas)
    poses = []
    for k in range(assoc.used.shape[0]):
        poses.append(T.copy())
        st = rr._step(v, P, N, assoc.used[k], assoc.rows[k], assoc.clipped[k], T, deltas[k], damp)
        if st is not None:
            T = gr.se3_exp(st[-1]) @ T
    return T, np.stack(poses)


def adjoint(v, P, N, assoc, T0, T_bar, deltas=None, damp=1e-8, poses=None, dtype=np.float64):
    """picp_robust_ref.adjoint with per-iteration frozen thresholds: (v_bar, P_bar, N_bar, T0_bar)"""
    v, P, N = (np.asarray(x, dtype) for x in (v, P, N))
    deltas = _frozen(assoc, deltas)
    if poses is None:
        _, poses = forward(v, P, N, assoc, T0, deltas, damp, dtype)
    poses = np.asarray(poses, dtype)
    Tb = np.zeros((4, 4), dtype)
    Tb[:3] = np.asarray(T_bar, dtype)[:3]
    vb, Pb, Nb = np.zeros_like(v), np.zeros_like(P), np.zeros_like(N)
    for k in range(assoc.used.shape[0] - 1, -1, -1):
        Tk = poses[k]
        st = rr._step(v, P, N, assoc.used[k], assoc.rows[k], assoc.clipped[k], Tk, deltas[k], damp)
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


def scaled_by(fx, f):
    """the fixture with every length multiplied by f (a power of two: exact): depth, vertex, map points, the translation
    of every pose; dist_thresh has to be scaled by the caller"""
    fx = dict(fx)
    for k in ("depth", "vertex", "points"):
        fx[k] = np.asarray(fx[k], F) * F(f)
    for k in ("model_pose", "T0", "gt"):
        if k in fx:
            T = np.array(fx[k], F)
            T[:3, 3] *= F(f)
            fx[k] = T
    return fx
