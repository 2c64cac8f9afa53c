"""Cases and float32 yardsticks of the projective ICP's backward pass, shared by tests/test_picp_backward_cpu.py (CPU)
and tests/test_hip_picp_backward.py (GPU).  No test lives here.

Every case is a deterministic function of its name: a fixture of the forward's tests (tests/picp_ref.convergence_fixture,
the edge fixture of tests/test_hip_picp.py), bent by `_bend` so that it meets every reject code and has map rows shared
by several slots, the solve's arguments and a standard-normal upstream adjoint of the pose.  (The edge fixture lives in a
test module marked `gpu`; importing it needs no GPU, and that module is the only home it has: this file depends on
`tests.test_hip_picp.edge_fixture` keeping its signature.)
The association and the float32 poses come from the restated forward (tests/picp_grad_ref.association), the adjoint from
tests/picp_grad_ref.adjoint evaluated at those poses.

Yardstick, as in tests/backward_cases.py and tests/render_backward_cases.py: the gap of a case is the distance between
the float32 and the float64 evaluation of the SAME NumPy adjoint, `rel_err` of tests/backward_cases.py (largest error over
all elements of an output relative to its largest element), per output (vertex_bar, points_bar, normals_bar,
init_pose_bar).  The gaps measured on the CPU are the constants GAP below (regenerate: python -m
tests.picp_backward_cases); the CPU suite recomputes them and fails when one has drifted by more than DRIFT, the GPU suite
allows the kernel kernel_bound(gap).  No bound is derived from a kernel's output."""
import functools

import numpy as np

from tests import picp_grad_ref as gr
from tests import picp_ref as pr
from tests.backward_cases import rel_err, weights

OUTPUTS = ("vertex_bar", "points_bar", "normals_bar", "init_pose_bar")

# name: (fixture, stride, numiters, dist_thresh).  At strides 3 and 4 neighbouring lattice slots are about 0.25 m apart on
# the surface, so two of them can only share a map row under a distance gate wider than that: those cases run with 0.5 m.
CASES = {
    "conv_s1": ("conv", 1, 10, 0.1),        # 60 x 80, 4 800 slots, 19 chunks
    "conv_s4": ("conv", 4, 10, 0.5),        # 300 slots, 2 chunks
    "conv_s4_n1": ("conv", 4, 1, 0.5),
    "conv_s1_n1": ("conv", 1, 1, 0.1),
    "edge_s3": ("edge3", 3, 6, 0.5),        # 37 x 53: 234 slots, one partial chunk; every reject code, stale entries, a
    "edge_s1": ("edge1", 1, 6, 0.1),        # device count below the bound; stride 1: 1 961 slots, 7 chunks and a tail
    "stale_dc": ("stale", 2, 5, 0.1),       # the index image of a longer map: 400 stale rows behind a device-side count
    "radius1": ("radius1", 1, 5, 0.1),      # index image rendered with radius 1: one surfel behind up to nine pixels
    "conv_t2": ("conv257", 1, 2, 0.1),      # 257 x 257: 66 049 slots, 259 chunks = two tiles of the scalar stage's column sum
}
NO_INLIER = ("no_winner", "no_depth")    # numiters 3, stride 1: the adjoint passes through
KW = dict(damp=1e-8, dist_thresh=0.1, angle_thresh=30.0)


class Case:
    pass


def _fixture(which):
    if which == "conv":
        fx = dict(pr.convergence_fixture())
    elif which == "conv257":
        fx = dict(pr.convergence_fixture(257, 257))
    elif which in ("edge3", "edge1"):
        from tests.test_hip_picp import edge_fixture
        fx = dict(edge_fixture(37, 53, 3 if which == "edge3" else 1))
        fx["T0"] = fx["T"]               # the pose at which the fixture meets every reject code
    elif which == "stale":
        fx = dict(pr.convergence_fixture(60, 80, 3, "facets"))
        fx["count"] = fx["count"] - 400  # (the buffers keep their rows: the bound is 400 above the device count)
    elif which == "radius1":
        from tests import render_ref as rr
        fx = dict(pr.convergence_fixture())
        P, N = fx["points"], fx["normals"]
        fx["index"] = rr.render(P, N, np.zeros_like(P), np.ones((P.shape[0], 1), np.float32), fx["model_pose"], fx["K"],
                                60, 80, radius=1).index
    elif which == "no_winner":
        fx = dict(pr.convergence_fixture())
        fx["index"] = np.full_like(fx["index"], -1)
    elif which == "no_depth":
        fx = dict(pr.convergence_fixture())
        fx["depth"] = np.zeros_like(fx["depth"])
    else:
        raise KeyError(which)
    return fx


SHARED_PAIRS = 8


def _bend(fx, stride, dist_thresh):
    """Makes the first linearisation (at T0) of a fixture meet what every case must exercise, changing only what it lacks:
    a slot of each reject code, in the manner of the edge fixture -- a zeroed depth (1), a live vertex moved 100 m
    sideways, out of the model view (2), a -1 hole in the index image (3), an associated map point moved two gates away (4),
    an associated normal flipped (5) -- and SHARED_PAIRS map rows used by two slots each: the index entry that a used
    slot reads is copied to the pixel its right-hand neighbour on the lattice reads, as a splat of radius >= 1 would
    (a radius-0 render shows a surfel in ONE pixel, so without this only a change of viewpoint at stride 1 makes two
    slots share a row).  Everything is verified afterwards from the restated forward (`claims`)."""
    from oracle import oracle as o
    for k in ("depth", "vertex", "points", "normals", "index"):
        fx[k] = np.array(fx[k])
    T0 = np.array(fx["T0"], np.float32)
    H, W = fx["depth"].shape
    Wl = (W + stride - 1) // stride
    r = pr.rows(*pr.args_of(fx), T0, stride=stride, dist_thresh=dist_thresh)
    used = np.nonzero(r.code == 0)[0]
    assert used.size > 60
    pix = o.project_map(o.transform_points(gr.lattice(fx["vertex"], stride), T0), fx["model_pose"], fx["K"], H, W)
    have = set(np.unique(r.code).tolist())
    picks = [int(used[(i + 1) * used.size // 7]) for i in range(5)]
    at = lambda k: ((k // Wl) * stride, (k % Wl) * stride)      # noqa: E731
    flat = fx["index"].reshape(-1)
    if 1 not in have:
        fx["depth"][at(picks[0])] = 0.0
    if 2 not in have:
        fx["vertex"][at(picks[1])][0] += np.float32(100.0)
    if 3 not in have:
        flat[int(pix[picks[2]])] = -1
    if 4 not in have:
        fx["points"][r.row[picks[3]], 1] += np.float32(2 * dist_thresh)
    if 5 not in have:
        fx["normals"][r.row[picks[4]]] *= np.float32(-1.0)
    # pairs of used slots side by side on the lattice, away from the slots bent above
    taken = set(picks) | {k + 1 for k in picks} | {k - 1 for k in picks}
    is_used = np.zeros(r.code.shape[0] + 1, bool)
    is_used[used] = True
    cand = [int(k) for k in used if (k + 1) % Wl != 0 and is_used[k + 1] and pix[k] != pix[k + 1]]
    cand = [k for k in cand if not ({k, k + 1} & taken)]
    done, last = 0, -10
    for k in cand[:: max(1, len(cand) // (4 * SHARED_PAIRS))]:
        if done == SHARED_PAIRS or k - last < 2:
            continue
        flat[int(pix[k + 1])] = r.row[k]
        done, last = done + 1, k
    assert done == SHARED_PAIRS, done
    return fx


@functools.lru_cache(maxsize=None)
def build(name):
    """The case as a namespace: fx (the forward's arguments), stride, numiters, device_count (None: the bound is exact),
    kw (damp and the two gates), assoc (picp_grad_ref.Association), v (ns, 3) lattice vertices, T_bar (4, 4) float32."""
    which, stride, numiters, dist_thresh = CASES[name] if name in CASES else (name, 1, 3, KW["dist_thresh"])
    c = Case()
    c.name, c.stride, c.numiters = name, stride, numiters
    c.kw = dict(KW, dist_thresh=dist_thresh)
    c.fx = _fixture(which)
    if name in CASES:
        c.fx = _bend(c.fx, stride, dist_thresh)
    c.device_count = c.fx["count"] if c.fx["count"] < c.fx["points"].shape[0] else None
    c.assoc = gr.association(*pr.args_of(c.fx), c.fx["T0"], stride=stride, numiters=numiters, **c.kw)
    c.v = gr.lattice(c.fx["vertex"], stride)
    c.T_bar = weights((4, 4), 31)
    return c


def reference(c, dtype=np.float64):
    """(vertex_bar (H, W, 3): zero off the lattice, points_bar, normals_bar, init_pose_bar) by the NumPy adjoint at the
    taped float32 poses"""
    vb, Pb, Nb, Tb = gr.adjoint(c.v, c.fx["points"], c.fx["normals"], c.assoc, c.fx["T0"], c.T_bar, damp=KW["damp"],
                                poses=c.assoc.poses, dtype=dtype)
    H, W = c.fx["depth"].shape
    full = np.zeros((H, W, 3), dtype)
    full[::c.stride, ::c.stride] = vb.reshape(full[::c.stride, ::c.stride].shape)
    return full, Pb, Nb, Tb


def claims(c):
    """What EVERY case must exercise, asserted from the reference alone: inliers in every iteration; a map row used by
    two or more slots in some iteration (the float64 atomics of the map scatter collide; radius1: by four or more); at
    least one slot of each of the codes 1 .. 5; an iteration whose association differs from the one before (numiters >
    1); with a device count, a stale index entry that a slot reads."""
    shared = 0
    for k in range(c.numiters):
        r = c.assoc.rows[k][c.assoc.used[k]]
        assert r.size > 20, "%s: iteration %d has %d inliers" % (c.name, k, r.size)
        shared = max(shared, int(np.bincount(r).max()))
    assert shared >= (4 if c.name == "radius1" else 2), "%s: no map row is used by several slots" % c.name
    assert set(np.unique(c.assoc.codes)) == {0, 1, 2, 3, 4, 5}, "%s: codes %s" % (c.name, np.unique(c.assoc.codes))
    if c.device_count is not None:
        assert (np.asarray(c.fx["index"]) >= c.device_count).any(), "%s: no stale entry" % c.name
    if c.numiters > 1:
        assert any((c.assoc.rows[k] != c.assoc.rows[k - 1]).any() for k in range(1, c.numiters)), \
            "%s: the association never changes" % c.name


def gaps(name):
    c = build(name)
    r64, r32 = reference(c), reference(c, np.float32)
    return tuple(rel_err(a, b) for a, b in zip(r32, r64))


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)
    'conv_s1': (6.4e-06, 1.7e-05, 3.4e-05, 2.3e-06),
    'conv_s4': (2.9e-05, 3.2e-05, 1.4e-04, 1.6e-06),
    'conv_s4_n1': (2.7e-06, 2.9e-06, 6.9e-06, 3.8e-06),
    'conv_s1_n1': (3.1e-06, 3.1e-06, 3.3e-06, 3.4e-06),
    'edge_s3': (5.9e-05, 5.9e-05, 5.9e-05, 1.9e-05),
    'edge_s1': (7.2e-06, 7.2e-06, 3.9e-05, 6.1e-07),
    'stale_dc': (1.3e-04, 1.3e-04, 5.2e-04, 2.3e-06),
    'radius1': (5.3e-05, 2.5e-05, 4.2e-05, 3.9e-07),
    'conv_t2': (1.9e-05, 1.3e-05, 1.5e-04, 5.3e-06),
}
# GAPS-END


if __name__ == "__main__":
    print("GAP = {   # case: (vertex_bar, points_bar, normals_bar, init_pose_bar)")
    for k in CASES:
        print("    %r: (%s)," % (k, ", ".join("%.1e" % x for x in gaps(k))))
    print("}")
