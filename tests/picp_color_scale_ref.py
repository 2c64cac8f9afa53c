"""Restatement of the joint projective ICP's COLOUR Huber threshold from the colour residuals' median (the
*_color_joint_scaled_* entry points: gs_picp_scale.hip in front of the robust kernel of gs_picp_color.hip) in NumPy, on top
of tests/picp_color_ref.py (the colour row), tests/picp_robust_ref.py (weights and terms) and tests/picp_scale_ref.py
(the selection and the constant).  TEST INFRASTRUCTURE ONLY.

Per iteration, at the pose T the iteration linearises at, with r the float32 colour residuals BEFORE color_weight is
applied (picp_color_ref.color_slot_rows with weight 1: 1.0f * r == r) of the slots that have a colour row (`colored`):

    med_c  = the LOWER median of |r|: the element of 0-based rank (n - 1) // 2 in ascending order (picp_scale_ref.select)
    c      = float32(color_huber_k) * float32(1.4826)     (picp_scale_ref.constant)
    cdelta = c * med_c (one float32 product); the floor (color_huber_delta) where the product is not above it (a NaN
             included)
    n == 0: cdelta = the floor               (the geometric rule gives +0.0 there; no weight is read in either case)

color_huber_k == 0: cdelta is the constant color_huber_delta.  The geometric threshold is picp_scale_ref.scale with
huber_k > 0 and the constant huber_delta otherwise.  Weights and terms are tests/picp_robust_ref.py's."""
import collections

import numpy as np

from tests import picp_color_ref as pcr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr

F = np.float32
o = pr.o
K_HUBER = sr.K_HUBER
Rows = collections.namedtuple("Rows", rr.ColorRows._fields + ("r", "delta", "cdelta"))


def color_scale(r, colored, color_huber_k, floor=0.0):
    """float32 colour threshold of one linearisation: max(c * lower median |r[colored]|, floor); the floor without a
    coloured slot, with a median of 0 and with color_huber_k == 0"""
    if not color_huber_k > 0:
        return F(floor)
    med, n = sr.lower_median_abs(r, colored)
    if n == 0:
        return F(floor)
    with np.errstate(invalid="ignore", over="ignore"):
        d = sr.constant(color_huber_k) * med
        assert d.dtype == F
        return d if d > F(floor) else F(floor)


def geometric_scale(b, used, huber_k, floor=0.0):
    """the geometric threshold: the median rule with huber_k > 0 (picp_scale_ref.scale), else the constant"""
    return sr.scale(b, used, huber_k, floor) if huber_k > 0 else F(floor)


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight, huber_k=0.0,
         huber_delta=0.0, color_huber_k=0.0, color_huber_delta=0.0, stride=1, dist_thresh=0.1, angle_thresh=30.0):
    """one weighted joint linearisation at T with the thresholds derived there: picp_robust_ref.ColorRows plus r (the
    colour residual before the weight, 0 where not coloured), delta and cdelta"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                   dot_th)
    used = code == 0
    ac, bc, colored = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight)
    _, r, _ = pcr.color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, 1.0)
    delta = geometric_scale(b, used, huber_k, huber_delta)
    cdelta = color_scale(r, colored, color_huber_k, color_huber_delta)
    w = rr.slot_weights(b, delta, used)
    wc = rr.slot_weights(r, cdelta, colored)
    sums = pr.reduce_terms(rr.terms(code, a, b, w) + rr.terms(code, ac, bc, wc))
    return Rows(code, row, a, b, ac, bc, colored, sums, int(used.sum()), int(colored.sum()), w, wc, r, delta, cdelta)


def color_solve(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T0, weight,
                huber_k=0.0, huber_delta=0.0, color_huber_k=0.0, color_huber_delta=0.0, stride=1, numiters=10, damp=1e-8,
                dist_thresh=0.1, angle_thresh=30.0):
    """(pose, trace (numiters, 9), deltas (numiters,), cdeltas (numiters,))"""
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 9), F)
    deltas, cdeltas = np.zeros(numiters, F), np.zeros(numiters, F)
    for it in range(numiters):
        q = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight, huber_k,
                 huber_delta, color_huber_k, color_huber_delta, stride, dist_thresh, angle_thresh)
        deltas[it], cdeltas[it] = q.delta, q.cdelta
        xi = np.zeros(6, F)
        if q.count > 0:
            xi = pr.solve_spd6(q.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:8], trace[it, 8] = F(q.count), F(q.sums[27]), xi, F(q.color_count)
    return T, trace, deltas, cdeltas


# ------------------------------------------------------------------------------------------ fixtures
def residual_fixture(h, w, e, used, ok=None, seed=5):
    """A scene in which the colour residual of pixel i is e[i] EXACTLY: identity live and model poses, a fronto-parallel
    plane at z = 1 whose vertices are the unprojected pixel centres (focal length 64 and an integer principal point: a
    pixel projects onto itself without rounding, u - w2 = v - h2 = 0), index = arange, map row i = vertex i (every
    geometric residual is 0), a black live frame (Il = 0) and a model intensity image with I = -e, so that
    r = 0 - ((-e + gx * 0) + gy * 0) = e.  gx, gy: small random values (they do not reach r, they do reach the colour
    rows); ok (h, w) bool: by default the interior pixels, which is what a view with every pixel hit has.  used (h * w)
    bool: the depth elsewhere is 0.  A slot is coloured where used & ok."""
    f, cx, cy = 64.0, float(w // 2), float(h // 2)
    Kc = np.eye(4, dtype=F)
    Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2] = f, f, cx, cy
    hh, ww = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    vertex = np.stack([(ww - F(cx)) / F(f), (hh - F(cy)) / F(f), np.ones((h, w), F)], -1).astype(F)
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    depth = np.where(np.asarray(used, bool).reshape(h, w), F(1.0), F(0.0)).astype(F)
    if ok is None:
        ok = interior(h, w)
    rng = np.random.default_rng(seed)
    model = np.zeros((h, w, 4), F)
    model[..., 0] = -np.asarray(e, F).reshape(h, w)
    model[..., 1] = np.where(ok, rng.uniform(-0.05, 0.05, (h, w)), 0.0).astype(F)
    model[..., 2] = np.where(ok, rng.uniform(-0.05, 0.05, (h, w)), 0.0).astype(F)
    model[..., 3] = ok
    eye = np.eye(4, dtype=F)
    return dict(vertex=vertex, normal=normal, depth=depth, K=Kc, index=np.arange(h * w, dtype=np.int64).reshape(h, w),
                model_pose=eye, points=vertex.reshape(-1, 3).copy(), normals=normal.reshape(-1, 3).copy(), count=h * w,
                color=np.zeros((h, w, 3), F), model=model, T=eye, T0=eye)


def interior(h, w):
    """(h, w) bool: the pixels whose four neighbours are inside the image"""
    ok = np.zeros((h, w), bool)
    ok[1:-1, 1:-1] = True
    return ok


def scaled_colors(fx, f):
    """the fixture with every colour multiplied by f (a power of two: exact): the live colour and the colour image of
    the model view, whose intensity image is built again (a fixture without that image: I, gx, gy times f, which is the
    same thing -- scaling by a power of two commutes with every rounding of luma and of the differences); color_weight
    has to be divided by f by the caller"""
    fx = dict(fx)
    fx["color"] = np.asarray(fx["color"], F) * F(f)
    if "view_color" in fx:
        fx["view_color"] = np.asarray(fx["view_color"], F) * F(f)
        fx["model"] = pcr.model_intensity(fx["view_color"], fx["index"])
    else:
        model = np.array(fx["model"], F)
        model[..., :3] *= F(f)
        fx["model"] = model
    return fx


BLOCK = rr.BLOCK                            # 15 % of a 60 x 80 image
BRIGHTER = 0.35                             # added to the live colour in the block: a specular / exposure patch


def brightened_block(fx, block=BLOCK, gain=BRIGHTER):
    """a copy of a textured fixture whose live COLOUR is `gain` brighter in `block` (the geometry is untouched)"""
    fx = dict(fx)
    color = np.array(fx["color"], F)
    color[block] = color[block] + F(gain)
    fx["color"] = color
    return fx
