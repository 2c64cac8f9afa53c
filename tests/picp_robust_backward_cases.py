"""Cases and float32 yardsticks of the projective ICP's backward pass WITH HUBER WEIGHTS, shared by
tests/test_picp_robust_cpu.py (CPU) and tests/test_hip_picp_robust.py (GPU).  No test lives here.

The scheme is that of tests/picp_backward_cases.py, whose fixtures and `_bend` are used as they are: every case meets every
reject code and has map rows shared by several slots.  On top of that each case has its own Huber threshold DELTA[name]
(metres), the first value of GRID (python -m tests.picp_robust_backward_cases --search) for which the restated forward
(tests/picp_robust_ref.association) satisfies `claims`: at least 10 clipped and 10 unclipped used slots in every
iteration, a map row shared by a clipped and an unclipped slot, and no used slot of any iteration within 1e-6 m of the
threshold (the kernel and the restatement then agree on every clip flag whatever the last bit of b).
The Gauss-Newton iterations converge fast: the first linearisation sees residuals of centimetres, the third one of a
tenth of a millimetre, and on a lattice of a few hundred slots no constant threshold leaves 10 slots on either side of
it in both.  The small lattices (edge_s3, edge_s1, conv_s4) therefore run TWO iterations -- the adjoint still crosses an
iteration boundary -- while conv_s1 (10) and stale_dc (5) have enough slots to keep both kinds to the end.

Yardstick: the gap of a case is the distance between the float32 and the float64 evaluation of the SAME NumPy adjoint
(tests/picp_robust_ref.adjoint at the taped float32 poses), `rel_err` of tests/backward_cases.py, per output.  The gaps
measured on the CPU are the constants GAP below (regenerate: python -m tests.picp_robust_backward_cases); the CPU suite
recomputes them and fails when one has drifted by more than DRIFT, the GPU suite allows the kernel kernel_bound(gap).  No
bound is derived from a kernel's output."""
import functools

import numpy as np

from tests import picp_backward_cases as pc
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests.backward_cases import rel_err, weights

OUTPUTS = pc.OUTPUTS

# name: (fixture, stride, numiters, dist_thresh) -- as in tests/picp_backward_cases.py
CASES = {
    "edge_s3": ("edge3", 3, 2, 0.5),        # 37 x 53: 234 slots, one partial chunk
    "edge_s1": ("edge1", 1, 2, 0.1),        # 1 961 slots: 7 chunks and a tail
    "conv_s1": ("conv", 1, 10, 0.1),        # 60 x 80: 4 800 slots, 19 chunks
    "conv_s4": ("conv", 4, 2, 0.5),         # 300 slots, 2 chunks
    "stale_dc": ("stale", 2, 5, 0.1),       # 400 stale rows behind a device count below the bound
}
NO_INLIER = pc.NO_INLIER                    # numiters 3, stride 1: the adjoint passes through
NO_INLIER_DELTA = 0.005
KW = pc.KW
MARGIN = 1e-6                               # no used slot has ||b| - delta| below this (metres)
GRID = tuple(round(0.005 - 0.000037 * i, 6) for i in range(125))   # 5 mm down to 0.4 mm

# DELTAS-BEGIN
DELTA = {
    'edge_s3': 0.00352,
    'edge_s1': 0.001115,
    'conv_s1': 0.004926,
    'conv_s4': 0.005,
    'stale_dc': 0.002114,
}
# DELTAS-END


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _bent(name):
    which, stride, numiters, dist_thresh = CASES[name]
    return pc._bend(pc._fixture(which), stride, dist_thresh)


def build(name, delta=None):
    """The case as a namespace: the fields of tests/picp_backward_cases.build, plus delta; assoc carries the clip flags"""
    if delta is None:
        return _build(name)
    which, stride, numiters, dist_thresh = CASES[name]
    c = Case()
    c.name, c.stride, c.numiters, c.delta = name, stride, numiters, float(delta)
    c.kw = dict(KW, dist_thresh=dist_thresh)
    c.fx = _bent(name)
    return _finish(c)


@functools.lru_cache(maxsize=None)
def _build(name):
    if name in CASES:
        return build(name, DELTA[name])
    c = Case()
    c.name, c.stride, c.numiters, c.delta = name, 1, 3, NO_INLIER_DELTA
    c.kw = dict(KW)
    c.fx = pc._fixture(name)
    return _finish(c)


def _finish(c):
    c.device_count = c.fx["count"] if c.fx["count"] < c.fx["points"].shape[0] else None
    c.assoc = rr.association(*pr.args_of(c.fx), c.fx["T0"], c.delta, stride=c.stride, numiters=c.numiters, **c.kw)
    c.v = rr.gr.lattice(c.fx["vertex"], c.stride)
    c.T_bar = weights((4, 4), 31)
    return c


def reference(c, dtype=np.float64):
    """(vertex_bar (H, W, 3): zero off the lattice, points_bar, normals_bar, init_pose_bar) by the NumPy adjoint at the
    taped float32 poses"""
    vb, Pb, Nb, Tb = rr.adjoint(c.v, c.fx["points"], c.fx["normals"], c.assoc, c.fx["T0"], c.T_bar, c.delta,
                                damp=KW["damp"], poses=c.assoc.poses, dtype=dtype)
    H, W = c.fx["depth"].shape
    full = np.zeros((H, W, 3), dtype)
    full[::c.stride, ::c.stride] = vb.reshape(full[::c.stride, ::c.stride].shape)
    return full, Pb, Nb, Tb


def residuals(c, k):
    """float32 b of iteration k's linearisation (zeros where the slot is not used)"""
    return pr.rows(*pr.args_of(c.fx), c.assoc.poses[k], stride=c.stride, dist_thresh=c.kw["dist_thresh"],
                   angle_thresh=c.kw["angle_thresh"]).b


def claims(c):
    """What EVERY case must exercise, asserted from the reference alone: the claims of tests/picp_backward_cases.py
    (inliers, shared rows, every reject code, a changing association, stale entries), and for the weights: at least 10
    clipped and 10 unclipped used slots in every iteration; a map row shared by a clipped and an unclipped slot in some
    iteration; no used slot of any iteration within MARGIN of the threshold."""
    pc.claims(c)
    mixed = False
    for k in range(c.numiters):
        used, clip = c.assoc.used[k], c.assoc.clipped[k]
        assert not (clip & ~used).any()
        n_clip, n_free = int(clip.sum()), int((used & ~clip).sum())
        assert n_clip >= 10 and n_free >= 10, "%s: iteration %d has %d clipped, %d unclipped" % (c.name, k, n_clip, n_free)
        b = residuals(c, k)[used].astype(np.float64)
        near = np.abs(np.abs(b) - float(np.float32(c.delta))).min()
        assert near >= MARGIN, "%s: iteration %d has a residual %.3g m from the threshold" % (c.name, k, near)
        r = c.assoc.rows[k]
        mixed = mixed or bool(np.intersect1d(r[clip], r[used & ~clip]).size)
    assert mixed, "%s: no map row is shared by a clipped and an unclipped slot" % c.name


def gaps(name):
    c = build(name)
    r64, r32 = reference(c), reference(c, np.float32)
    return tuple(rel_err(a, b) for a, b in zip(r32, r64))


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)
    'edge_s3': (3.2e-04, 3.2e-04, 1.4e-03, 4.5e-05),
    'edge_s1': (1.3e-03, 1.4e-03, 1.1e-03, 3.9e-05),
    'conv_s1': (6.3e-05, 9.7e-05, 1.5e-04, 1.7e-06),
    'conv_s4': (2.8e-05, 3.4e-05, 7.5e-05, 2.8e-06),
    'stale_dc': (4.0e-05, 4.4e-05, 3.3e-04, 2.8e-06),
}
# GAPS-END


def _search(name):
    """the first threshold of GRID that satisfies `claims`"""
    for delta in GRID:
        try:
            claims(build(name, delta))
            return delta
        except AssertionError as e:
            print("#   %s: delta %g fails: %s" % (name, delta, e))
    raise RuntimeError("no threshold found for " + name)


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        print("DELTA = {")
        for k in CASES:
            print("    %r: %r," % (k, _search(k)))
        print("}")
    else:
        print("GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)")
        for k in CASES:
            print("    %r: (%s)," % (k, ", ".join("%.1e" % x for x in gaps(k))))
        print("}")
