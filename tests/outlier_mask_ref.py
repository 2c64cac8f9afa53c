"""Restatement of the projective ICP's outlier mask (gs_picp_outliers.hip: the class pass behind
gs_picp_outlier_classes_batch_f32 and the region pass behind gs_region_mask_u8) in NumPy, on top of tests/picp_ref.py,
picp_scale_ref.py and picp_weighted_ref.py.  TEST INFRASTRUCTURE ONLY.

The rule, per sequence, at a float32 pose T, over EVERY pixel of the live frame (stride 1 whatever the solve's stride):

    1  association   code, b of each pixel: picp_weighted_ref.slot_rows at T with stride 1 (a pixel the weights mask has
                     code 6)
    2  scale         med = the lower median of |b| over the code-0 pixels (picp_scale_ref: the kernel's radix selection);
                     hi_t = scale(b, used, hi, floor), lo_t = scale(b, used, lo, floor): one float32 product
                     (float)k * 1.4826f, one product with med, then the floor; +0.0 without a used pixel.  A threshold
                     of 0 makes no pixel strong or eligible by its residual
    3  classes       strong   = (code == 0 and |b| > hi_t and hi_t > 0) or code == 4 or code == 5
                     eligible = strong or (code == 0 and |b| > lo_t and lo_t > 0)
                     strict float32 comparisons; codes 1, 2, 3 and 6 have class 0.  The class byte: bit 0 strong, bit 1
                     eligible
    4  support       seed(p) = strong(p) and at least min_support of the 3 x 3 window around p are strong (p counts;
                     pixels outside the image do not)
    5  growth        M_0 = seed;  M_{i+1}(p) = M_i(p) or (eligible(p) and some 4-neighbour q inside the image has M_i(q)
                     and |depth(p) - depth(q)| <= grow_depth), one float32 subtraction, then fabs; exactly `grow` steps.
                     The mask is M_grow, uint8 0 / 1."""
import collections

import numpy as np

from tests import picp_ref as pr
from tests import picp_scale_ref as sr
from tests import picp_weighted_ref as wr

F = np.float32
STRONG, ELIGIBLE = 1, 2
DEFAULTS = dict(hi=3.0, lo=1.5, floor=0.0, min_support=6, grow=0, grow_depth=0.02)
Outliers = collections.namedtuple("Outliers", ["mask", "classes", "thresholds", "code", "b"])


def thresholds(b, used, hi=3.0, lo=1.5, floor=0.0):
    """float32 (hi_t, lo_t): picp_scale_ref.scale of the two constants"""
    return np.array([sr.scale(b, used, hi, floor), sr.scale(b, used, lo, floor)], F)


def classes(code, b, hi_t, lo_t):
    """uint8 class bytes of per-pixel codes and float32 residuals (any shape)"""
    code, ab = np.asarray(code), np.abs(np.asarray(b, F))
    hi_t, lo_t = F(hi_t), F(lo_t)
    with np.errstate(invalid="ignore"):
        strong = ((code == 0) & (ab > hi_t) & bool(hi_t > 0)) | (code == 4) | (code == 5)
        eligible = strong | ((code == 0) & (ab > lo_t) & bool(lo_t > 0))
    return (strong * STRONG + eligible * ELIGIBLE).astype(np.uint8)


def _padded(x, fill=0):
    p = np.full((x.shape[0] + 2, x.shape[1] + 2), fill, x.dtype)
    p[1:-1, 1:-1] = x
    return p


def seeds(cls, min_support=6):
    """bool (H, W): strong pixels with at least min_support strong pixels in their 3 x 3 window"""
    strong = (np.asarray(cls, np.uint8) & STRONG) != 0
    p = _padded(strong.astype(np.int32))
    H, W = strong.shape
    n = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return strong & (n >= int(min_support))


def region_mask(cls, depth, min_support=6, grow=0, grow_depth=0.02):
    """uint8 (H, W) mask of one class image and its float32 depth"""
    cls, depth = np.asarray(cls, np.uint8), np.asarray(depth, F)
    assert cls.shape == depth.shape and cls.ndim == 2
    H, W = cls.shape
    eligible = (cls & ELIGIBLE) != 0
    gd = F(grow_depth)
    M = seeds(cls, min_support)
    dp = _padded(depth)
    for _ in range(int(grow)):
        Mp = _padded(M)
        reach = np.zeros((H, W), bool)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            q = Mp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]            # (False outside the image)
            with np.errstate(invalid="ignore"):
                diff = np.abs(depth - dp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
            assert diff.dtype == F
            with np.errstate(invalid="ignore"):
                reach |= q & (diff <= gd)
        M = M | (eligible & reach)
    return M.astype(np.uint8)


def outliers(vertex, normal, depth, K, index, model_pose, points, normals, count, T, weights=None, hi=3.0, lo=1.5,
             floor=0.0, min_support=6, grow=0, grow_depth=0.02, dist_thresh=0.1, angle_thresh=30.0):
    """the rule at T for one sequence: Outliers(mask (H, W) uint8, classes (H, W) uint8, thresholds (2,) float32, code
    (H, W) int32, b (H, W) float32)"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, _, _, b, _ = wr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, weights, T, 1,
                                    dist_th, dot_th)
    shape = np.asarray(depth).shape
    th = thresholds(b, code == 0, hi, lo, floor)
    cls = classes(code, b, th[0], th[1]).reshape(shape)
    return Outliers(region_mask(cls, depth, min_support, grow, grow_depth), cls, th, code.reshape(shape),
                    b.reshape(shape))


def masked_weights(mask, weights=None):
    """the refinement's weight image: the caller's weights, or ones, 0 where masked"""
    w = np.ones(mask.shape, F) if weights is None else np.array(weights, F)
    w[np.asarray(mask) != 0] = 0
    return w


def refine(fx, solve_kw, stride, first_iters=10, refine_iters=5, weights=None, **rule):
    """first solve / the mask at its pose / refine_iters more iterations, plain and masked, from that pose.  Returns
    (T_first, T_plain, T_masked, Outliers)"""
    args = pr.args_of(fx)
    T1 = wr.solve(*args, weights, fx["T0"], stride=stride, numiters=first_iters, **solve_kw)[0]
    out = outliers(*args, T1, weights, **rule)
    Tp = wr.solve(*args, weights, T1, stride=stride, numiters=refine_iters, **solve_kw)[0]
    Tm = wr.solve(*args, masked_weights(out.mask, weights), T1, stride=stride, numiters=refine_iters, **solve_kw)[0]
    return T1, Tp, Tm, out
