"""Inputs, cases and float32 yardsticks shared by tests/test_backward_oracles_cpu.py (CPU) and
tests/test_hip_backward_kernels.py (GPU).  No test lives here.

Every case is a deterministic function of its key.  The yardstick of a float32 kernel on one input is the distance
between the float32 and the float64 evaluation of the SAME numpy adjoint (oracle/maps_backward.py) on that input:
`gap = max |f32 - f64| / max |f64|` over all elements.  The gaps measured on the CPU are the constants *_GAP below
(regenerate: python -m tests.backward_cases); the CPU suite recomputes every one of them and fails when a constant
has drifted, the GPU suite allows a kernel KERNEL_FACTOR x the constant of the case (its gather order and its
specified exp polynomial differ from numpy's), never less than FLOOR_ULPS float32 ulps of the scale.  No bound is
derived from a kernel's output."""
import functools

import numpy as np

SIGMA = 0.6
KERNEL_FACTOR = 4.0
FLOOR_ULPS = 8.0
EPS32 = float(np.finfo(np.float32).eps)
DRIFT = 1.5            # a recomputed gap must lie within [constant / DRIFT, constant * DRIFT]

FRAME_SIZES = [(2, 2), (2, 300), (300, 2), (67, 131), (259, 517), (480, 640)]
FRAME_VARIANTS = [("fy+", "asis"), ("fy-", "asis"), ("fy+", "clamp"), ("fy-", "clamp")]
FRAME_LOSSES = ["v", "n", "a", "vna"]
GLOBAL_LOSSES = ["gv", "gn", "gvgn"]
ALPHA_SIZES = [255, 256, 257, 100003]
CLAMP_RADIUS = 3.4066  # |v| at which exp(-|v|^2 / (2 * 0.6^2)) crosses the 1e-7 clamp: sqrt(0.72 ln 1e7)


def rel_err(got, ref):
    """Largest error over ALL elements relative to the largest reference element."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def kernel_bound(gap):
    return max(KERNEL_FACTOR * gap, FLOOR_ULPS * EPS32)


@functools.lru_cache(maxsize=None)
def _surface(seed):
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(1, 480, 640, seed=seed, hole_frac=0.0)
    return s["depths"][0, ..., 0].copy(), s["intrinsics"][0].copy(), s["poses"][0].copy()


def frame_case(H, W, fy="fy+", scale="asis", seed=21):
    """(depth (H, W) float32, K (4, 4) float32).  A crop of the smooth synthetic surface with a rectangular hole, 2 %
    isolated invalid pixels, the top third of the last column invalid and the right quarter of the last row negative.
    (Only PART of the last column / row: an invalid pixel's normal carries no gradient, so a border that is invalid
    throughout would switch the border terms of the adjoint off instead of testing them.)
    scale == "clamp": depth scaled so that the median |vertex| is CLAMP_RADIUS, valid pixels on both sides of the
    alpha clamp."""
    surf, K, _ = _surface(seed)
    oh, ow = (480 - H) // 2, (640 - W) // 2
    depth = surf[oh:oh + H, ow:ow + W].astype(np.float64)
    K = K.copy()
    K[0, 2] -= ow
    K[1, 2] -= oh
    if fy == "fy-":
        K[1, 1] = -K[1, 1]
    if scale == "clamp":
        w, h = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        ray = np.sqrt(((w - K[0, 2]) / K[0, 0]) ** 2 + ((h - K[1, 2]) / K[1, 1]) ** 2 + 1.0)
        depth = depth * (CLAMP_RADIUS / np.median(ray * depth))
    rng = np.random.default_rng([seed, H, W])
    depth[rng.random((H, W)) < 0.02] = 0.0
    depth[H // 3:H // 3 + H // 4, W // 2:W // 2 + W // 5] = 0.0
    depth[:H // 3, W - 1] = 0.0
    depth[H - 1, W - W // 4:] *= -1.0
    return depth.astype(np.float32), K.astype(np.float32)


def generic_pose():
    from oracle.icp_backward import se3_exp
    return se3_exp(np.array([0.4, -0.3, 0.2, 0.5, -0.7, 0.3])).astype(np.float32)


def weights(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def frame_weights(H, W, loss):
    """(v_bar, n_bar, a_bar): standard normal where the loss uses the map, zero elsewhere."""
    wv, wn, wa = weights((H, W, 3), 1), weights((H, W, 3), 2), weights((H, W), 3)
    return (wv if "v" in loss else np.zeros_like(wv), wn if "n" in loss else np.zeros_like(wn),
            wa if "a" in loss else np.zeros_like(wa))


def frame_key(H, W, fy, scale, loss):
    return "%dx%d/%s/%s/%s" % (H, W, fy, scale, loss)


def alpha_points(n):
    """(n, 3) float32 points whose norms straddle the clamp radius (2.4 .. 4.4 m) plus a few near the origin."""
    rng = np.random.default_rng([5, n])
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 2.4 + 2.0 * rng.random(n)
    r[::17] = 0.05 * rng.random(len(r[::17]))
    return (d * r[:, None]).astype(np.float32)


# ----------------------------------------------------------------------------------------------- gap measurement
def frame_gaps(H, W, fy, scale, loss):
    """(depth_bar gap, K_bar gap) of the frame-map adjoint on this case."""
    from oracle import maps_backward as mb
    depth, K = frame_case(H, W, fy, scale)
    vb, nb, ab = frame_weights(H, W, loss)
    d64, k64 = mb.frame_maps_backward(depth, K, SIGMA, vb, nb, ab, want_K=True)
    d32, k32 = mb.frame_maps_backward(depth, K, SIGMA, vb, nb, ab, want_K=True, dtype=np.float32)
    return rel_err(d32, d64), rel_err(k32, k64)


def local_maps(depth, K):
    """float32 vertex and normal maps of a case, by the float64 forward of the oracle rounded once."""
    from oracle import maps_backward as mb
    V, N, _ = mb.frame_maps_forward(depth, K, SIGMA)
    return V.astype(np.float32), N.astype(np.float32)


def global_gaps(H, W, loss):
    """(v_bar gap, n_bar gap, pose_bar gap) of the global-map adjoint; None where the loss leaves an output out."""
    from oracle import maps_backward as mb
    depth, K = frame_case(H, W)
    v, n = local_maps(depth, K)
    gvb = weights((H, W, 3), 4) if "gv" in loss else None
    gnb = weights((H, W, 3), 5) if "gn" in loss else None
    r64 = mb.global_maps_backward(v, n, depth, generic_pose(), gvb, gnb)
    r32 = mb.global_maps_backward(v, n, depth, generic_pose(), gvb, gnb, dtype=np.float32)
    return tuple(None if a is None else rel_err(a, b) for a, b in zip(r32, r64))


def alpha_gaps(n):
    from oracle import maps_backward as mb
    p, ab = alpha_points(n), weights((n,), 6)
    p64, s64 = mb.alpha_backward(p, SIGMA, 1e-7, ab)
    p32, s32 = mb.alpha_backward(p, SIGMA, 1e-7, ab, dtype=np.float32)
    return rel_err(p32, p64), abs(float(s32) - float(s64)) / abs(float(s64))


def measure_all():
    frame = {}
    for H, W in FRAME_SIZES:
        for fy, scale in FRAME_VARIANTS:
            for loss in FRAME_LOSSES:
                frame[frame_key(H, W, fy, scale, loss)] = frame_gaps(H, W, fy, scale, loss)
    glob = {"%dx%d/%s" % (H, W, loss): global_gaps(H, W, loss) for H, W in FRAME_SIZES for loss in GLOBAL_LOSSES}
    alpha = {n: alpha_gaps(n) for n in ALPHA_SIZES}
    return frame, glob, alpha


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
FRAME_GAP = {   # key: (depth_bar, K_bar)
    '2x2/fy+/asis/v': (2.3e-08, 2.6e-08),
    '2x2/fy+/asis/n': (6.8e-08, 9.1e-05),
    '2x2/fy+/asis/a': (4.7e-07, 4.6e-07),
    '2x2/fy+/asis/vna': (5.4e-08, 6.5e-06),
    '2x2/fy-/asis/v': (4.4e-08, 2.2e-08),
    '2x2/fy-/asis/n': (7.5e-08, 2.0e-05),
    '2x2/fy-/asis/a': (4.7e-07, 4.6e-07),
    '2x2/fy-/asis/vna': (5.7e-08, 2.0e-05),
    '2x2/fy+/clamp/v': (2.3e-08, 3.2e-08),
    '2x2/fy+/clamp/n': (1.1e-07, 1.9e-04),
    '2x2/fy+/clamp/a': (3.4e-07, 3.2e-07),
    '2x2/fy+/clamp/vna': (1.9e-08, 2.2e-05),
    '2x2/fy-/clamp/v': (4.4e-08, 2.8e-08),
    '2x2/fy-/clamp/n': (3.4e-08, 1.2e-04),
    '2x2/fy-/clamp/a': (3.4e-07, 3.2e-07),
    '2x2/fy-/clamp/vna': (3.6e-08, 4.6e-06),
    '2x300/fy+/asis/v': (2.7e-08, 1.3e-07),
    '2x300/fy+/asis/n': (6.4e-06, 2.2e-05),
    '2x300/fy+/asis/a': (2.9e-07, 1.3e-06),
    '2x300/fy+/asis/vna': (6.4e-06, 5.3e-05),
    '2x300/fy-/asis/v': (2.9e-08, 1.3e-07),
    '2x300/fy-/asis/n': (5.9e-06, 8.6e-05),
    '2x300/fy-/asis/a': (2.9e-07, 1.3e-06),
    '2x300/fy-/asis/vna': (5.9e-06, 4.3e-05),
    '2x300/fy+/clamp/v': (2.7e-08, 2.3e-07),
    '2x300/fy+/clamp/n': (4.5e-06, 5.3e-05),
    '2x300/fy+/clamp/a': (5.5e-07, 1.5e-06),
    '2x300/fy+/clamp/vna': (4.6e-06, 6.5e-05),
    '2x300/fy-/clamp/v': (2.9e-08, 2.2e-07),
    '2x300/fy-/clamp/n': (5.3e-06, 4.1e-05),
    '2x300/fy-/clamp/a': (5.5e-07, 1.5e-06),
    '2x300/fy-/clamp/vna': (5.3e-06, 3.3e-05),
    '300x2/fy+/asis/v': (3.2e-08, 1.3e-07),
    '300x2/fy+/asis/n': (7.4e-06, 2.9e-05),
    '300x2/fy+/asis/a': (5.5e-07, 2.0e-07),
    '300x2/fy+/asis/vna': (7.4e-06, 1.6e-05),
    '300x2/fy-/asis/v': (3.4e-08, 1.3e-07),
    '300x2/fy-/asis/n': (1.4e-05, 1.0e-04),
    '300x2/fy-/asis/a': (5.5e-07, 2.1e-07),
    '300x2/fy-/asis/vna': (1.4e-05, 3.9e-05),
    '300x2/fy+/clamp/v': (3.2e-08, 1.0e-07),
    '300x2/fy+/clamp/n': (9.7e-06, 1.5e-04),
    '300x2/fy+/clamp/a': (9.8e-07, 3.2e-07),
    '300x2/fy+/clamp/vna': (9.7e-06, 1.1e-05),
    '300x2/fy-/clamp/v': (3.4e-08, 1.0e-07),
    '300x2/fy-/clamp/n': (1.3e-05, 1.5e-04),
    '300x2/fy-/clamp/a': (9.8e-07, 3.2e-07),
    '300x2/fy-/clamp/vna': (1.3e-05, 6.6e-06),
    '67x131/fy+/asis/v': (3.6e-08, 2.7e-07),
    '67x131/fy+/asis/n': (4.0e-06, 2.2e-05),
    '67x131/fy+/asis/a': (5.2e-07, 6.6e-07),
    '67x131/fy+/asis/vna': (4.0e-06, 7.6e-05),
    '67x131/fy-/asis/v': (3.6e-08, 2.7e-07),
    '67x131/fy-/asis/n': (4.4e-06, 1.9e-04),
    '67x131/fy-/asis/a': (5.2e-07, 6.6e-07),
    '67x131/fy-/asis/vna': (4.4e-06, 7.1e-05),
    '67x131/fy+/clamp/v': (3.6e-08, 2.0e-07),
    '67x131/fy+/clamp/n': (4.6e-06, 1.1e-04),
    '67x131/fy+/clamp/a': (7.7e-07, 4.4e-07),
    '67x131/fy+/clamp/vna': (4.6e-06, 2.2e-05),
    '67x131/fy-/clamp/v': (3.6e-08, 2.0e-07),
    '67x131/fy-/clamp/n': (3.5e-06, 5.7e-05),
    '67x131/fy-/clamp/a': (7.7e-07, 4.4e-07),
    '67x131/fy-/clamp/vna': (3.5e-06, 5.6e-05),
    '259x517/fy+/asis/v': (6.3e-08, 3.1e-08),
    '259x517/fy+/asis/n': (2.5e-05, 1.5e-04),
    '259x517/fy+/asis/a': (6.0e-07, 2.4e-06),
    '259x517/fy+/asis/vna': (2.5e-05, 3.0e-05),
    '259x517/fy-/asis/v': (5.6e-08, 3.1e-08),
    '259x517/fy-/asis/n': (1.8e-05, 9.7e-05),
    '259x517/fy-/asis/a': (6.0e-07, 2.4e-06),
    '259x517/fy-/asis/vna': (1.8e-05, 1.8e-05),
    '259x517/fy+/clamp/v': (6.3e-08, 1.6e-07),
    '259x517/fy+/clamp/n': (2.1e-05, 1.7e-04),
    '259x517/fy+/clamp/a': (7.7e-07, 4.2e-06),
    '259x517/fy+/clamp/vna': (2.1e-05, 1.7e-05),
    '259x517/fy-/clamp/v': (5.6e-08, 1.6e-07),
    '259x517/fy-/clamp/n': (1.9e-05, 7.9e-05),
    '259x517/fy-/clamp/a': (7.7e-07, 4.2e-06),
    '259x517/fy-/clamp/vna': (2.0e-05, 8.8e-06),
    '480x640/fy+/asis/v': (7.9e-08, 1.4e-07),
    '480x640/fy+/asis/n': (3.5e-05, 4.9e-05),
    '480x640/fy+/asis/a': (4.6e-07, 2.5e-06),
    '480x640/fy+/asis/vna': (3.6e-05, 2.1e-05),
    '480x640/fy-/asis/v': (7.1e-08, 1.4e-07),
    '480x640/fy-/asis/n': (3.5e-05, 5.7e-05),
    '480x640/fy-/asis/a': (4.6e-07, 2.5e-06),
    '480x640/fy-/asis/vna': (3.5e-05, 1.2e-05),
    '480x640/fy+/clamp/v': (7.9e-08, 1.6e-07),
    '480x640/fy+/clamp/n': (3.3e-05, 6.4e-05),
    '480x640/fy+/clamp/a': (6.2e-07, 4.7e-07),
    '480x640/fy+/clamp/vna': (3.3e-05, 8.5e-06),
    '480x640/fy-/clamp/v': (7.1e-08, 1.6e-07),
    '480x640/fy-/clamp/n': (3.0e-05, 9.0e-05),
    '480x640/fy-/clamp/a': (6.2e-07, 4.7e-07),
    '480x640/fy-/clamp/vna': (3.0e-05, 2.7e-05),
}
GLOBAL_GAP = {   # key: (v_bar, n_bar, pose_bar)
    '2x2/gv': (2.4e-08, None, 3.6e-08),
    '2x2/gn': (None, 6.7e-08, 1.0e-07),
    '2x2/gvgn': (2.4e-08, 6.7e-08, 3.0e-08),
    '2x300/gv': (5.0e-08, None, 2.5e-07),
    '2x300/gn': (None, 7.7e-08, 4.5e-07),
    '2x300/gvgn': (5.0e-08, 7.7e-08, 2.1e-07),
    '300x2/gv': (4.5e-08, None, 1.9e-07),
    '300x2/gn': (None, 7.7e-08, 2.6e-07),
    '300x2/gvgn': (4.5e-08, 7.7e-08, 1.8e-07),
    '67x131/gv': (6.9e-08, None, 2.2e-06),
    '67x131/gn': (None, 6.1e-08, 1.7e-06),
    '67x131/gvgn': (6.9e-08, 6.1e-08, 2.1e-06),
    '259x517/gv': (6.6e-08, None, 4.2e-06),
    '259x517/gn': (None, 6.8e-08, 7.1e-06),
    '259x517/gvgn': (6.6e-08, 6.8e-08, 3.0e-06),
    '480x640/gv': (7.3e-08, None, 6.4e-06),
    '480x640/gn': (None, 7.4e-08, 7.7e-06),
    '480x640/gvgn': (7.3e-08, 7.4e-08, 6.3e-06),
}
ALPHA_GAP = {   # n: (points_bar, sigma_bar)
    255: (9.2e-08, 2.4e-07),
    256: (6.1e-08, 1.9e-07),
    257: (8.6e-08, 4.7e-06),
    100003: (1.3e-07, 1.6e-06),
}
# GAPS-END


if __name__ == "__main__":
    def fmt(t):
        return "(" + ", ".join("None" if x is None else "%.1e" % x for x in t) + ")"
    frame, glob, alpha = measure_all()
    print("FRAME_GAP = {   # key: (depth_bar, K_bar)")
    for k, v in frame.items():
        print("    %r: %s," % (k, fmt(v)))
    print("}\nGLOBAL_GAP = {   # key: (v_bar, n_bar, pose_bar)")
    for k, v in glob.items():
        print("    %r: %s," % (k, fmt(v)))
    print("}\nALPHA_GAP = {   # n: (points_bar, sigma_bar)")
    for k, v in alpha.items():
        print("    %r: %s," % (k, fmt(v)))
    print("}")
