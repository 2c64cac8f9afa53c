"""Cases of the model view with per-surfel radii, forward and backward, shared by tests/test_radii_cpu.py (CPU) and
tests/test_hip_radii.py (GPU).  No test lives here.

Maps (oracle frame loop with the SurfelRadii layer rule between the frames, tests/radii_ref.run_sequence, ground-truth
odometry): `wave` = frame 0 of make_sequence(2, 60, 80, seed=0, scene="wave"), 4 556 rows; `odd` = 3 frames of
make_sequence(3, 37, 53, seed=3).  Views: "0" = sequence pose 0, "o1" = render_backward_cases.off_pose(pose 1),
"z+0.4" = pose 0 moved by 0.4 m along its optical axis.  Radii: "layer" = the fused radii; "span" = radii chosen so that
in the FIRST view row n has half-width n mod 10 before the cap (every r of 0 ... max_radius occurs), with rows 5 ... 8
set to 0, -1, NaN and +inf and the rows 100 ... 119 appended once more at the end (equal depths: the lower row wins).

Backward yardstick, as in tests/render_backward_cases.py: the gap of a case is the distance between the float32 and the
float64 evaluation of the same NumPy adjoint (tests/render_grad_ref.adjoint on the restated index image), per output;
the constants GAP are measured on the CPU (regenerate: python -m tests.render_radii_backward_cases), the CPU suite
recomputes them and fails on drift, the GPU suite allows backward_cases.kernel_bound(gap)."""
import functools

import numpy as np

from tests import radii_ref
from tests import render_grad_ref as gr
from tests import render_radii_ref as rrr
from tests import render_ref as rr
from tests.backward_cases import rel_err, weights
from tests.render_backward_cases import off_pose

OUTPUTS = ("points_bar", "normals_bar", "poses_bar")


@functools.lru_cache(maxsize=None)
def scene(which):
    """(sequence dict, oracle map, layer) of a map"""
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(2, 60, 80, seed=0, scene="wave") if which == "wave" else make_sequence(3, 37, 53, seed=3)
    L = 1 if which == "wave" else 3
    m, lay = radii_ref.run_sequence(s["colors"][:L], s["depths"][:L], s["intrinsics"][0], s["poses"][:L])
    if which == "wave":
        assert len(m) == 4556
    assert len(m) <= 5000
    return s, m, lay


def view_pose(s, v):
    if v[0] == "o":
        return off_pose(s["poses"][int(v[1:])])
    if v[0] == "z":
        return rrr.moved(s["poses"][0], float(v[1:]))
    return s["poses"][int(v)]


# name: (map, views, radii, max_radius, render arguments, upstream adjoints, rows counted on the device or None)
V5 = ("0", "z+0.4", "z+1.0", "o1", "z-2.0")          # 5 > 4 views: two launches
CASES = {
    "layer_near": ("wave", ("z+0.4", "0", "z+1.0"), "layer", 3, {}, "zcof", None),
    "span_cap8": ("wave", V5, "span", 8, {}, "zcof", None),
    "span_cap3": ("wave", ("0", "o1", "z+0.4", "z+1.0"), "span", 3, {}, "zcof", None),
    "cap0": ("wave", ("z+0.4",), "layer", 0, {}, "zcof", None),
    "filters": ("wave", ("o1", "z+0.4"), "span", 3, {"min_confidence": "median", "cull_backfaces": "flip"}, "zcof", None),
    "odd_count": ("odd", ("o1", "z-1.5"), "span", 8, {}, "zcof", -37),
    "only_z": ("wave", ("z+0.4", "0", "z+1.0"), "layer", 3, {}, "z", None),
    "only_c": ("wave", ("z+0.4", "0", "z+1.0"), "layer", 3, {}, "c", None),
}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """The case as a namespace: points / normals / colors / ccounts / radii (float32; every row of the buffers), n (the
    rows that are the map: the device-side count of the case, else all), poses (L, 4, 4), K, H, W, max_radius, kw (the
    two filters), index / depth (L, H, W) and images (per view the Rendered) of the restated forward, r (L, n) the
    half-width of every row per view, pix (L, n) its pixel or -1, upstream adjoints zb / cb / ob / fb."""
    which, views, rad, cap, kw, ups, short = CASES[name]
    s, m, lay = scene(which)
    c = Case()
    c.name, c.max_radius = name, cap
    c.H, c.W = s["depths"].shape[1:3]
    c.K = s["intrinsics"][0].astype(np.float32)
    c.poses = np.stack([view_pose(s, v) for v in views]).astype(np.float32)
    P, N, C, F = (np.ascontiguousarray(getattr(m, k), np.float32) for k in ("points", "normals", "colors", "ccounts"))
    radii = lay.radius.copy()
    c.dups = None
    if rad == "span":
        _, key = rr.row_keys(P, N, F, c.poses[0], c.K, c.H, c.W)
        z = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        k = (np.arange(len(P)) % 10).astype(np.float32)
        with np.errstate(all="ignore"):
            radii = (((k + np.float32(0.5)) * z) / radii_ref.fbar_of(c.K)).astype(np.float32)
        radii[5:9] = (0.0, -1.0, np.nan, np.inf)
        dup = np.arange(100, 120)
        c.dups = (dup, len(P) + np.arange(len(dup)))
        P, N, C, F, radii = (np.concatenate([a, a[dup]]) for a in (P, N, C, F, radii))
    c.kw = dict(kw)
    if c.kw.get("cull_backfaces") == "flip":
        # the fused normals point away from the cameras that saw them: flip every third, so that the test keeps some
        N = N.copy()
        N[::3] = -N[::3]
        c.kw["cull_backfaces"] = True
    if c.kw.get("min_confidence") == "median":
        cc = np.sort(F.reshape(-1))
        c.kw["min_confidence"] = float(cc[len(cc) // 2])
    c.points, c.normals, c.colors, c.ccounts, c.radii = P, N, C, F, radii
    c.n = len(P) if short is None else len(P) + short
    n, L = c.n, len(views)
    out = [rrr.render(P[:n], N[:n], C[:n], F[:n], radii[:n], c.poses[v], c.K, c.H, c.W, cap, **c.kw) for v in range(L)]
    c.images = [o_[0] for o_ in out]
    c.r = np.stack([o_[1] for o_ in out])
    c.pix = np.stack([rrr.row_splats(P[:n], N[:n], F[:n], radii[:n], c.poses[v], c.K, c.H, c.W, cap, **c.kw)[0]
                      for v in range(L)])
    c.index = np.stack([i.index for i in c.images])
    c.depth = np.stack([i.depth[..., 0] for i in c.images])
    shape = (L, c.H, c.W)
    c.zb = weights(shape, 21) if "z" in ups else None
    c.cb = weights(shape + (3,), 22) if "c" in ups else None
    c.ob = weights(shape + (3,), 23) if "o" in ups else None
    c.fb = weights(shape, 24) if "f" in ups else None
    return c


def reference(c, dtype=np.float64):
    """(points_bar, normals_bar, colors_bar, ccounts_bar, poses_bar) over the first c.n rows by the NumPy adjoint"""
    n = c.n
    return gr.adjoint(c.points[:n], c.normals[:n], c.poses, c.index, c.zb, c.cb, c.ob, c.fb, dtype=dtype)


def claims(c):
    """What a case must exercise, asserted on the restated forward."""
    L, n = c.index.shape[0], c.n
    per_view = []
    for v in range(L):
        idx, live = c.index[v], c.pix[v] >= 0
        assert (idx >= 0).mean() > 0.1, "%s: view %d does not show the scene" % (c.name, v)
        per_view.append(np.bincount(idx[idx >= 0], minlength=n))
        assert c.r[v][live].max() <= c.max_radius and c.r[v][~live].max(initial=0) == 0
    assert (c.index < 0).any(), "%s: no empty pixel" % c.name
    won = np.stack(per_view)
    assert (won.sum(0) == 0).any(), "%s: every row wins a pixel" % c.name
    if c.max_radius >= 1:
        assert len(np.unique(c.r[c.pix >= 0])) >= min(c.max_radius + 1, 3), "%s: the radii do not mix" % c.name
        if L >= 2:
            assert (((won >= 2).sum(0)) >= 2).any(), "%s: no row wins several pixels in several views" % c.name
        else:
            assert won.max() >= 2
    else:
        assert won.max() == 1
    if CASES[c.name][2] == "span":
        live = c.pix[0] >= 0
        assert set(np.unique(c.r[0][live])) == set(range(c.max_radius + 1)), "%s: not every r in view 0" % c.name
        assert not c.r[:, 5:9].any(), "%s: radii 0, negative, NaN, inf give r = 0" % c.name
        orig, dup = c.dups
        if not c.kw:
            h, w, r = c.pix[0][live] // c.W, c.pix[0][live] % c.W, c.r[0][live]
            assert (h - r < 0).any() and (h + r > c.H - 1).any() and (w - r < 0).any() and (w + r > c.W - 1).any(), \
                "%s: no row is clipped at some border" % c.name
        if dup.max() < n and not c.kw:
            assert (c.pix[0][orig] >= 0).any() and np.array_equal(c.pix[:, orig], c.pix[:, dup])
            assert np.isin(c.index[0], orig).any() and not np.isin(c.index, dup).any(), \
                "%s: a tie is not settled towards the lower row" % c.name
    if "min_confidence" in c.kw:
        plain = rrr.render(c.points[:n], c.normals[:n], c.colors[:n], c.ccounts[:n], c.radii[:n], c.poses[0], c.K, c.H,
                           c.W, c.max_radius)[0]
        assert not np.array_equal(plain.index, c.index[0]), "%s: the filters change nothing" % c.name


def gaps(name):
    """(points_bar, normals_bar, poses_bar) gaps of the case: float32 against float64 NumPy; None: the output is zero."""
    c = build(name)
    r64, r32 = reference(c), reference(c, np.float32)
    return tuple(rel_err(r32[i], r64[i]) if np.abs(r64[i]).max() > 0 else None for i in (0, 1, 4))


# ----------------------------------------------------------------------------------------------- measured gaps
# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
GAP = {   # case: (points_bar, normals_bar, poses_bar)
    'layer_near': (1.1e-07, 9.7e-08, 1.4e-06),
    'span_cap8': (3.7e-07, 3.4e-07, 1.3e-06),
    'span_cap3': (2.0e-07, 2.2e-07, 1.7e-06),
    'cap0': (0.0e+00, 0.0e+00, 9.4e-07),
    'filters': (1.7e-07, 1.1e-07, 1.3e-06),
    'odd_count': (2.9e-07, 4.3e-07, 5.4e-07),
    'only_z': (1.1e-07, None, 1.5e-06),
    'only_c': (None, None, None),
}
# GAPS-END


if __name__ == "__main__":
    print("GAP = {   # case: (points_bar, normals_bar, poses_bar)")
    for k in CASES:
        claims(build(k))
        print("    %r: (%s)," % (k, ", ".join("None" if x is None else "%.1e" % x for x in gaps(k))))
    print("}")
