"""Cases and float32 yardsticks of the projective ICP's backward pass WITH THE THRESHOLD FROM THE RESIDUALS' MEDIAN,
shared by tests/test_picp_scale_cpu.py (CPU) and tests/test_hip_picp_scale.py (GPU).  No test lives here.

The scheme is that of tests/picp_robust_backward_cases.py, whose bent fixtures are used as they are (every case meets
every reject code and has map rows shared by several slots).  There is no threshold to search for: the forward derives
one per iteration (tests/picp_scale_ref.association with huber_k = 1.345 and no floor), and by construction of the
median it leaves clipped and unclipped rows in every iteration, so the small lattices run three iterations here, not
two.  The thresholds are constants of the adjoint, one per iteration, frozen like the clip flags and the association.

Yardstick: the gap of a case is the distance between the float32 and the float64 evaluation of the SAME NumPy adjoint
(tests/picp_scale_ref.adjoint at the taped float32 poses), `rel_err` of tests/backward_cases.py, per output.  The gaps
measured on the CPU are the constants GAP below (regenerate: python -m tests.picp_scale_backward_cases); the CPU suite
recomputes them and fails when one has drifted by more than DRIFT, the GPU suite allows the kernel kernel_bound(gap).  No
bound is derived from a kernel's output."""
import functools

import numpy as np

from tests import picp_backward_cases as pc
from tests import picp_ref as pr
from tests import picp_robust_backward_cases as rc
from tests import picp_scale_ref as sr
from tests.backward_cases import rel_err, weights

OUTPUTS = pc.OUTPUTS
HUBER_K = sr.K_HUBER

# name: (fixture, stride, numiters, dist_thresh) -- fixtures and gates as in tests/picp_robust_backward_cases.py
CASES = {
    "edge_s3": ("edge3", 3, 3, 0.5),        # 37 x 53: 234 slots, one partial chunk
    "edge_s1": ("edge1", 1, 3, 0.1),        # 1 961 slots: 7 chunks and a tail
    "conv_s1": ("conv", 1, 5, 0.1),         # 60 x 80: 4 800 slots, 19 chunks
    "conv_s4": ("conv", 4, 3, 0.5),         # 300 slots, 2 chunks
    "stale_dc": ("stale", 2, 3, 0.1),       # 400 stale rows behind a device count below the bound (the facets converge
}                                           # to residuals of 1e-7 m by iteration 4: float32 then measures nothing)
NO_INLIER = pc.NO_INLIER                    # numiters 3, stride 1: the adjoint passes through, every threshold is 0
KW = pc.KW
MIXED = ("edge_s1", "conv_s1", "conv_s4")     # some iteration has a map row shared by a clipped and an unclipped slot
assert all(CASES[k][0] == rc.CASES[k][0] and CASES[k][1] == rc.CASES[k][1] and CASES[k][3] == rc.CASES[k][3]
           for k in CASES)                  # (rc._bent bends a fixture for the stride and the gate of rc.CASES)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """The case as a namespace: the fields of tests/picp_backward_cases.build; assoc (picp_scale_ref.Association)
    carries the clip flags and the thresholds of every iteration"""
    c = Case()
    if name in CASES:
        which, stride, numiters, dist_thresh = CASES[name]
        c.kw = dict(KW, dist_thresh=dist_thresh)
        c.fx = rc._bent(name)
    else:
        stride, numiters = 1, 3
        c.kw = dict(KW)
        c.fx = pc._fixture(name)
    c.name, c.stride, c.numiters, c.huber_k = name, stride, numiters, HUBER_K
    c.device_count = c.fx["count"] if c.fx["count"] < c.fx["points"].shape[0] else None
    c.assoc = sr.association(*pr.args_of(c.fx), c.fx["T0"], c.huber_k, 0.0, stride=c.stride, numiters=c.numiters, **c.kw)
    c.v = sr.gr.lattice(c.fx["vertex"], c.stride)
    c.T_bar = weights((4, 4), 31)
    return c


def reference(c, dtype=np.float64):
    """(vertex_bar (H, W, 3): zero off the lattice, points_bar, normals_bar, init_pose_bar) by the NumPy adjoint at the
    taped float32 poses and thresholds"""
    vb, Pb, Nb, Tb = sr.adjoint(c.v, c.fx["points"], c.fx["normals"], c.assoc, c.fx["T0"], c.T_bar, damp=KW["damp"],
                                poses=c.assoc.poses, dtype=dtype)
    H, W = c.fx["depth"].shape
    full = np.zeros((H, W, 3), dtype)
    full[::c.stride, ::c.stride] = vb.reshape(full[::c.stride, ::c.stride].shape)
    return full, Pb, Nb, Tb


def claims(c):
    """What EVERY case must exercise, asserted from the reference alone: the claims of tests/picp_backward_cases.py
    (inliers, shared rows, every reject code, a changing association, stale entries); in EVERY iteration clipped and
    unclipped used slots, the clipped ones fewer than half (the median is not clipped); thresholds that differ between
    two iterations, all positive.  Returns whether some iteration has a map row shared by a clipped and an unclipped
    slot (there is no threshold to choose here, so not every case has one: MIXED names the ones that must)."""
    pc.claims(c)
    mixed = False
    for k in range(c.numiters):
        used, clip = c.assoc.used[k], c.assoc.clipped[k]
        assert not (clip & ~used).any()
        n_clip, n_free = int(clip.sum()), int((used & ~clip).sum())
        assert n_clip >= 10 and n_free >= 10, "%s: iteration %d has %d clipped, %d unclipped" % (c.name, k, n_clip, n_free)
        assert 2 * n_clip < n_clip + n_free
        r = c.assoc.rows[k]
        mixed = mixed or bool(np.intersect1d(r[clip], r[used & ~clip]).size)
    assert mixed or c.name not in MIXED, "%s: no map row is shared by a clipped and an unclipped slot" % c.name
    d = c.assoc.deltas
    assert d.dtype == np.float32 and (d > 0).all() and np.unique(d).size >= 2, "%s: thresholds %s" % (c.name, d)
    return mixed


def gaps(name):
    c = build(name)
    r64, r32 = reference(c), reference(c, np.float32)
    return tuple(rel_err(a, b) for a, b in zip(r32, r64))


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)
    'edge_s3': (4.6e-04, 4.8e-04, 2.9e-04, 2.0e-05),
    'edge_s1': (3.0e-04, 3.0e-04, 1.5e-04, 9.6e-06),
    'conv_s1': (8.3e-05, 8.2e-05, 1.4e-04, 3.7e-06),
    'conv_s4': (2.9e-04, 3.0e-04, 1.7e-04, 6.3e-06),
    'stale_dc': (4.2e-03, 4.1e-03, 4.4e-03, 1.9e-05),
}
# GAPS-END


if __name__ == "__main__":
    print("GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)")
    for k in CASES:
        print("#   %s: shared by a clipped and an unclipped slot: %s" % (k, claims(build(k))))
        print("    %r: (%s)," % (k, ", ".join("%.1e" % x for x in gaps(k))))
    print("}")
