"""CPU tests of the render backward: the NumPy adjoint (tests/render_grad_ref.py) against central finite differences of
a float64 forward with the winners held fixed, the committed float32 yardsticks of tests/render_backward_cases.py
against a fresh measurement, and the library's exports / register report for the new kernels.

The forward is linear in the points, in the translation and in the rotation entries separately, so a central difference
along one coordinate (or along any direction of ONE of the inputs) is exact up to float64 rounding: the bound is 1e-8
relative to the largest element of the adjoint it is compared with."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import backward_cases as bc
from tests import render_backward_cases as rc
from tests import render_grad_ref as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1e-8
FD_CASES = ["r0_seq", "r2_off", "neg_fy", "filters", "views3", "loss6"]


def _loss(c, points, normals, colors, ccounts, poses):
    depth, color, normal, conf = gr.forward(points, normals, colors, ccounts, poses, c.index)
    total = 0.0
    for img, up in ((depth, c.zb), (color, c.cb), (normal, c.ob), (conf, c.fb)):
        if up is not None:
            hit = c.index >= 0
            total += float((img[hit] * np.asarray(up, np.float64)[hit]).sum())
    return total


def _central(c, args, which, delta, h=0.5):
    a, b = [x.copy() for x in args], [x.copy() for x in args]
    a[which] = a[which] + h * delta
    b[which] = b[which] - h * delta
    return (_loss(c, *a) - _loss(c, *b)) / (2 * h)


@pytest.mark.parametrize("name", FD_CASES)
def test_reference_adjoint_equals_finite_differences(name):
    c = rc.build(name)
    rc.claims(c)
    args = [np.asarray(x, np.float64) for x in (c.points, c.normals, c.colors, c.ccounts.reshape(-1), c.poses)]
    pb, nb, cb, fb, Tb = gr.adjoint(c.points, c.normals, c.poses, c.index, c.zb, c.cb, c.ob, c.fb)
    assert not Tb[:, 3].any(), "the bottom row of the pose adjoint is exactly zero"
    won = np.zeros(len(c.points), bool)
    won[c.index[c.index >= 0]] = True
    for g in (pb, nb, cb, fb):
        assert not g[~won].any(), "rows that win nothing get exactly zero"
    rng = np.random.default_rng(7)
    winners, losers = np.nonzero(won)[0], np.nonzero(~won)[0]
    rows = np.concatenate([rng.choice(winners, 24, replace=False), rng.choice(losers, 4, replace=False)])
    worst = 0.0
    for which, g in ((0, pb), (1, nb), (2, cb), (3, fb)):
        scale = np.abs(g).max()
        if scale == 0:
            continue
        # coordinate by coordinate on sampled rows ...
        for r in rows:
            for k in range(g.shape[1] if g.ndim == 2 else 1):
                d = np.zeros_like(args[which])
                d[(r, k) if g.ndim == 2 else r] = 1.0
                fd = _central(c, args, which, d)
                err = abs(fd - (g[r, k] if g.ndim == 2 else g[r])) / scale
                worst = max(worst, err)
                assert err <= FD_BOUND, (name, which, int(r), k, fd, err)
        # ... and along random directions over all rows (a sum over every element of g: relative to its largest element)
        for _ in range(3):
            d = rng.standard_normal(g.shape)
            fd = _central(c, args, which, d)
            err = abs(fd - float((g * d).sum())) / scale
            worst = max(worst, err)
            assert err <= FD_BOUND, (name, which, "direction", fd, err)
    # every entry of the top three rows of every pose
    scale = np.abs(Tb).max()
    for v in range(Tb.shape[0]):
        for i in range(3):
            for j in range(4):
                d = np.zeros_like(args[4])
                d[v, i, j] = 1.0
                fd = _central(c, args, 4, d)
                err = abs(fd - Tb[v, i, j]) / scale
                worst = max(worst, err)
                assert err <= FD_BOUND, (name, "pose", v, i, j, fd, Tb[v, i, j], err)
    print("%s: worst finite-difference error %.2e (bound %.0e)" % (name, worst, FD_BOUND))


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_committed_gap_is_current(name):
    """the float32 yardstick the GPU suite uses is what this machine measures, within DRIFT"""
    c = rc.build(name)
    rc.claims(c)
    got, want = rc.gaps(name), rc.GAP[name]
    print(name, got, want)
    for out, g, w in zip(rc.OUTPUTS, got, want):
        assert (g is None) == (w is None), (name, out, g, w)
        if g is not None:
            assert w / bc.DRIFT <= g <= w * bc.DRIFT, (name, out, g, w)


def test_every_case_has_a_gap_and_upstream_alone_and_together():
    assert set(rc.GAP) == set(rc.CASES)
    ups = {v[5] for v in rc.CASES.values()}
    assert {"z", "c", "o", "f", "zcof"} <= ups
    assert {len(v[1]) for v in rc.CASES.values()} >= {1, 3, 9}
    assert {v[4].get("radius", 0) for v in rc.CASES.values()} >= {0, 1, 2}


def test_library_exports_the_backward_entry_points():
    from gradslam_amd import _C
    assert {"gs_render_backward_scratch_bytes", "gs_render_map_backward_dc_f32"} <= set(_C.EXPORTS)
    if not os.path.exists(_C.LIB_PATH):
        from gradslam_amd.csrc import build
        build.build()
    lib = _C.lib()
    assert hasattr(lib, "gs_render_map_backward_dc_f32") and hasattr(lib, "gs_render_backward_scratch_bytes")
    # 4 views x ceil(n / 256) partial rows of 12 float64 at least; views beyond 4 reuse them
    n = 2_000_000
    need = 4 * ((n + 255) // 256) * 12 * 8
    assert need <= lib.gs_render_backward_scratch_bytes(9, 480, 640, n) == lib.gs_render_backward_scratch_bytes(4, 480, 640, n)
    assert lib.gs_render_backward_scratch_bytes(1, 480, 640, n) >= need // 4
    assert lib.gs_render_backward_scratch_bytes(0, 480, 640, n) == 0
    # argument validation returns before any HIP call
    assert lib.gs_render_map_backward_dc_f32(None, 1, 1, 4, 4, 0, None) == 1
    seqs = (_C.RenderBackwardSeq * 1)()
    assert lib.gs_render_map_backward_dc_f32(seqs, 1, 1, 4, 4, 4, None) == 1 and b"radius" in lib.gs_last_error()
    assert lib.gs_render_map_backward_dc_f32(seqs, 1, 1, 4, 4, 0, None) == 1 and b"NULL" in lib.gs_last_error()


def test_backward_kernels_do_not_spill():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_render.hip",
                        "gs_rview_backward"], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if l and not l.startswith("#")]
    names = {row[-1] for row in rows}
    assert names == {"gs_rview_backward_rows_kernel", "gs_rview_backward_pose_kernel"}, r.stdout
    for vgpr, sgpr, scratch, occ, sspill, vspill, lds, name in rows:
        print(name, "VGPR", vgpr, "scratch", scratch, "occupancy", occ)
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
        assert re.fullmatch(r"\d+", occ) and int(occ) >= 4, (name, occ)
