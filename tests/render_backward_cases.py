"""Cases and float32 yardsticks of the render backward, shared by tests/test_render_backward_cpu.py (CPU) and
tests/test_hip_render_backward.py (GPU).  No test lives here.

Every case is a deterministic function of its name: one of the two maps of tests/test_hip_render.py (`small`: 96x128, 6
frames; `big`: 480x640, 2 frames; oracle frame loop, ground-truth odometry), views, intrinsics, render arguments and
standard-normal upstream adjoints.  The index image comes from the NumPy restatement of the forward
(tests/render_ref.render), the adjoint from tests/render_grad_ref.adjoint.

Yardstick, as in tests/backward_cases.py: the gap of a case is the distance between the float32 and the float64
evaluation of the SAME NumPy adjoint, `rel_err` of that module (largest error over all elements of an output relative
to its largest element), per output (points_bar, normals_bar, poses_bar; None where the loss leaves the output zero).
The gaps measured on the CPU are the constants GAP below (regenerate: python -m tests.render_backward_cases); the CPU
suite recomputes them and fails when one has drifted by more than DRIFT, the GPU suite allows the kernel
kernel_bound(gap) = max(KERNEL_FACTOR x gap, FLOOR_ULPS ulps).  No bound is derived from a kernel's output."""
import functools
import math

import numpy as np

from tests import render_grad_ref as gr
from tests import render_ref as rr
from tests.backward_cases import rel_err, weights

OUTPUTS = ("points_bar", "normals_bar", "poses_bar")


@functools.lru_cache(maxsize=None)
def scene(which):
    """(sequence dict, oracle map) as the `small` / `big` fixtures of tests/test_hip_render.py build them"""
    from gradslam_amd.datasets.synthetic import make_sequence
    from oracle import slam as oslam
    s = make_sequence(6, 96, 128, seed=0) if which == "small" else make_sequence(2, 480, 640, seed=5)
    m, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gt")
    if which == "small":
        assert len(m) == 20410
    return s, m


def off_pose(pose):
    """a pose that is not one of the sequence: 4 degrees of yaw and a translation on top of `pose`"""
    a = math.radians(4.0)
    D = np.eye(4, dtype=np.float64)
    D[0, 0], D[0, 2], D[2, 0], D[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    D[:3, 3] = (0.03, -0.02, 0.05)
    return (pose.astype(np.float64) @ D).astype(np.float32)


def mirrored_K(K, H):
    K = K.copy()
    K[1, 1], K[1, 2] = -K[1, 1], (H - 1) - K[1, 2]
    return K


def scaled_K(K, f):
    K = K.copy()
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K[0, 0] * f, K[1, 1] * f, K[0, 2] * f, K[1, 2] * f
    return K


# name: (map, views, K variant, rows (None: all), render arguments, upstream adjoints)
# views: "3" = sequence pose 3, "o1" = off_pose(sequence pose 1); upstream: z depth, c colour, o normal, f confidence,
# "residual" = the depth adjoint of metrics.render_loss against the sequence's frames
V3 = ("0", "3", "o5")
V9 = ("0", "1", "2", "3", "4", "5", "o0", "o2", "o5")     # 9 > 2 x 4 views: three launches
CASES = {
    "r0_seq": ("small", ("3",), "K", None, {}, "zcof"),
    "r1_off": ("small", ("o1",), "K", None, {"radius": 1}, "zcof"),
    "r2_off": ("small", ("o1",), "K", None, {"radius": 2}, "zcof"),
    "neg_fy": ("small", ("o4",), "mirrored", None, {"radius": 1}, "zcof"),
    "filters": ("small", ("o1",), "K", None, {"radius": 1, "min_confidence": "median", "cull_backfaces": True}, "zcof"),
    "views3": ("small", V3, "K", None, {"radius": 1}, "zcof"),
    "views3_r0": ("small", V3, "K", None, {}, "zcof"),
    "views9": ("small", V9, "K", None, {"radius": 1}, "zcof"),
    "ragged_9001": ("small", ("o0", "2", "4"), "scaled0.9", 9001, {"radius": 1}, "zcof"),
    "only_z": ("small", V3, "K", None, {"radius": 1}, "z"),
    "only_c": ("small", V3, "K", None, {"radius": 1}, "c"),
    "only_o": ("small", V3, "K", None, {"radius": 1}, "o"),
    "only_f": ("small", V3, "K", None, {"radius": 1}, "f"),
    "loss6": ("small", ("0", "1", "2", "3", "4", "5"), "K", None, {}, "residual"),
    "big_r0": ("big", ("1",), "K", None, {}, "zcof"),
    "big_r1_off": ("big", ("o1", "0"), "K", None, {"radius": 1}, "zcof"),
}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """The case as a namespace: points / normals / colors / ccounts (float32), poses (L, 4, 4), K, H, W, kw (render
    arguments), index (L, H, W) and depth (L, H, W) of the restated forward, upstream adjoints zb / cb / ob / fb
    (float32, or None)."""
    which, views, kvar, rows, kw, ups = CASES[name]
    s, m = scene(which)
    c = Case()
    c.name, c.seq = name, s
    n = len(m) if rows is None else rows
    c.points, c.normals, c.colors, c.ccounts = (np.ascontiguousarray(getattr(m, k)[:n], np.float32) for k in
                                                ("points", "normals", "colors", "ccounts"))
    c.H, c.W = s["depths"].shape[1:3]
    K = s["intrinsics"][0]
    c.K = {"K": K, "mirrored": mirrored_K(K, c.H), "scaled0.9": scaled_K(K, 0.9)}[kvar].astype(np.float32)
    c.poses = np.stack([off_pose(s["poses"][int(v[1:])]) if v[0] == "o" else s["poses"][int(v)] for v in views]).astype(np.float32)
    c.kw = dict(kw)
    if c.kw.get("min_confidence") == "median":
        cc = np.sort(c.ccounts.reshape(-1))
        c.kw["min_confidence"] = float(cc[len(cc) // 2])
    L = len(views)
    rendered = [rr.render(c.points, c.normals, c.colors, c.ccounts, c.poses[v], c.K, c.H, c.W, **c.kw) for v in range(L)]
    c.index = np.stack([r.index for r in rendered])
    c.depth = np.stack([r.depth[..., 0] for r in rendered])
    shape = (L, c.H, c.W)
    c.zb = c.cb = c.ob = c.fb = None
    if ups == "residual":
        fd = np.stack([s["depths"][int(v)][..., 0] for v in views]).astype(np.float64)
        rd = c.depth.astype(np.float64)
        both = (fd > 0) & (rd > 0)
        cnt = both.reshape(L, -1).sum(-1).astype(np.float64)
        c.zb = (np.where(both, rd - fd, 0.0) / np.maximum(cnt, 1.0)[:, None, None]).astype(np.float32)
        c.frame_depth, c.both = fd, both
    else:
        c.zb = weights(shape, 11) if "z" in ups else None
        c.cb = weights(shape + (3,), 12) if "c" in ups else None
        c.ob = weights(shape + (3,), 13) if "o" in ups else None
        c.fb = weights(shape, 14) if "f" in ups else None
    return c


def reference(c, dtype=np.float64):
    """(points_bar, normals_bar, colors_bar, ccounts_bar, poses_bar) of the case by the NumPy adjoint"""
    return gr.adjoint(c.points, c.normals, c.poses, c.index, c.zb, c.cb, c.ob, c.fb, dtype=dtype)


def claims(c):
    """What a case must exercise, asserted on the restated forward: some pixels are empty, every view shows the scene; a
    row that wins at least 2 pixels of a view at radius >= 1; a row that wins pixels in at least 2 views when there are."""
    L = c.index.shape[0]
    assert (c.index < 0).any(), "%s: no empty pixel" % c.name
    per_view = []
    for v in range(L):
        idx = c.index[v]
        assert (idx >= 0).mean() > 0.1, "%s: view %d does not show the scene" % (c.name, v)
        won = np.bincount(idx[idx >= 0], minlength=len(c.points))
        if c.kw.get("radius", 0) >= 1:
            assert won.max() >= 2, "%s: no row wins 2 pixels of view %d" % (c.name, v)
        per_view.append(won > 0)
    if L >= 2:
        assert (np.sum(per_view, axis=0) >= 2).any(), "%s: no row wins pixels in 2 views" % c.name
    assert (np.sum(per_view, axis=0) == 0).any(), "%s: every row wins a pixel" % c.name


def gaps(name):
    """(points_bar, normals_bar, poses_bar) gaps of the case: float32 against float64 NumPy; None: the output is zero."""
    c = build(name)
    r64, r32 = reference(c), reference(c, np.float32)
    out = []
    for i in (0, 1, 4):
        out.append(rel_err(r32[i], r64[i]) if np.abs(r64[i]).max() > 0 else None)
    return tuple(out)


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
GAP = {   # case: (points_bar, normals_bar, poses_bar)
    'r0_seq': (3.1e-08, 8.3e-08, 3.3e-06),
    'r1_off': (4.1e-08, 6.5e-08, 1.4e-06),
    'r2_off': (8.3e-08, 7.5e-08, 1.2e-06),
    'neg_fy': (6.1e-08, 9.1e-08, 1.3e-06),
    'filters': (8.1e-08, 7.3e-08, 1.2e-06),
    'views3': (9.3e-08, 1.1e-07, 2.0e-06),
    'views3_r0': (7.2e-08, 8.6e-08, 2.1e-06),
    'views9': (1.1e-07, 1.3e-07, 9.2e-07),
    'ragged_9001': (1.3e-07, 1.3e-07, 1.8e-06),
    'only_z': (9.3e-08, None, 1.4e-06),
    'only_c': (None, None, None),
    'only_o': (None, 1.1e-07, 2.1e-06),
    'only_f': (None, None, None),
    'loss6': (8.5e-08, None, 1.5e-06),
    'big_r0': (4.8e-08, 8.1e-08, 5.1e-06),
    'big_r1_off': (8.1e-08, 8.1e-08, 1.3e-05),
}
# GAPS-END


if __name__ == "__main__":
    print("GAP = {   # case: (points_bar, normals_bar, poses_bar)")
    for k in CASES:
        print("    %r: (%s)," % (k, ", ".join("None" if x is None else "%.1e" % x for x in gaps(k))))
    print("}")
