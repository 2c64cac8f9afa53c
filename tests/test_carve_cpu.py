"""CPU-only tests of the free-space carve: the NumPy restatement (tests/carve_ref.py) against hand-written cases, the
demonstration (a block of pixels that stands nearer to the camera for six frames and is then gone) on the oracle frame
loop with the restated carve between the frames, the host-side argument validation of gs_free_space_dc_f32 (it returns
before any HIP call), and the arguments of ops.free_space*, Pointclouds.carve_ / free_space_violations and
PointFusion(carve_*=...).

The rule's outputs are integers, so every comparison of them is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from gradslam_amd.slam.pointfusion import PointFusion
from gradslam_amd.structures.pointclouds import Pointclouds
from gradslam_amd.structures.rgbdimages import RGBDImages
from oracle import slam as oslam
from tests import carve_ref as cr
from tests import render_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
f32 = np.float32

# a camera at the origin looking down +z: a point (x, y, z) lands on pixel u = 10 x / z + 4, v = 10 y / z + 3
H, W = 7, 9
K = np.array([[10, 0, 4, 0], [0, 10, 3, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
EYE = np.eye(4, dtype=f32)


def at(h, w, z):
    """the point of depth z on the ray through the centre of pixel (h, w)"""
    return [(w - 4) * z / 10.0, (h - 3) * z / 10.0, z]


# ------------------------------------------------------------------------------------------ the restatement
def test_ref_margin_equality_and_one_ulp():
    z, margin = f32(1.0), f32(0.25)
    d_eq = f32(1.25)                                     # 1.25 - 1.0 == 0.25 exactly in float32
    assert f32(d_eq - z) == margin
    P = np.array([at(3, 4, z)], f32)
    for d, want in ((d_eq, False), (np.nextafter(d_eq, f32(9)), True), (np.nextafter(d_eq, f32(0)), False)):
        D = np.full((H, W), d, f32)
        assert cr.violates(P, D, EYE, K, margin, 0).tolist() == [want], d
        assert cr.violates(P, D, EYE, K, margin, 1).tolist() == [want], d
    # margin 0: a row exactly on the measured surface stays, one ulp in front of it goes
    D = np.full((H, W), z, f32)
    assert cr.violates(P, D, EYE, K, 0.0, 0).tolist() == [False]
    assert cr.violates(P, np.full((H, W), np.nextafter(z, f32(9)), f32), EYE, K, 0.0, 0).tolist() == [True]


def test_ref_centre_without_measurement_is_no_evidence():
    P = np.array([at(3, 4, 1.0)], f32)
    for hole in (0.0, -2.0, NAN, -0.0):
        D = np.full((H, W), 2.0, f32)
        D[3, 4] = hole
        for window in (0, 1, 2):
            assert cr.violates(P, D, EYE, K, 0.05, window).tolist() == [False], (hole, window)
    # an infinite depth is a measurement (inf > 0, inf - z > margin)
    D = np.full((H, W), np.inf, f32)
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [True]


def test_ref_nan_and_hidden_rows_never_violate():
    D = np.full((H, W), 5.0, f32)
    P = np.array([at(3, 4, 1.0), [NAN, 0, 1], [0, 0, NAN], at(3, 4, -1.0), [0, 0, 0], at(3, 40, 1.0), at(-30, 4, 1.0),
                  at(3, 4, 6.0)], f32)
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [True] + [False] * 7


def test_ref_window_holes_abstain_and_one_near_pixel_vetoes():
    P = np.array([at(3, 4, 1.0)], f32)
    D = np.full((H, W), 2.0, f32)
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [True]
    D[2, 3] = 0.0           # a hole in the window abstains
    D[4, 5] = NAN
    D[3, 5] = -1.0
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [True]
    D[4, 3] = 1.04          # one measured corner at the row's own depth: the row is next to a depth edge
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [False]
    assert cr.violates(P, D, EYE, K, 0.05, 0).tolist() == [True]
    D[4, 3] = 2.0
    D[1, 2] = 1.0           # outside window 1, inside window 2
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [True]
    assert cr.violates(P, D, EYE, K, 0.05, 2).tolist() == [False]


def test_ref_windows_are_clipped_at_every_border():
    D = np.full((H, W), 2.0, f32)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 4), (H - 1, 4), (3, 0), (3, W - 1)]
    P = np.array([at(h, w, 1.0) for h, w in corners], f32)
    for window in (0, 1, 2, 3):
        assert cr.violates(P, D, EYE, K, 0.05, window).all(), window
    # the veto pixel of a border row is found inside the clipped window, and not across the image edge (no wrap-around)
    D[1, W - 1] = 1.0
    got = cr.violates(P, D, EYE, K, 0.05, 1).tolist()
    assert got == [True, False, True, True, True, True, True, True]
    got = cr.violates(P, D, EYE, K, 0.05, 2).tolist()
    assert got == [True, False, True, True, True, True, True, False]


def test_ref_counts_views_and_min_views():
    P = np.array([at(3, 4, 1.0), at(2, 2, 1.0), at(3, 4, 3.0), [9, 9, 9]], f32)
    far, near = np.full((H, W), 2.0, f32), np.full((H, W), 1.0, f32)
    part = far.copy()
    part[1:4, 0:3] = 1.0     # covers the pixel of row 1, stays out of the window of row 0
    depths, poses = [far, near, part, far], [EYE] * 4
    viol, keep = cr.free_space(P, 3, depths, poses, K, 0.05, 1, 1)
    assert viol.tolist() == [3, 2, 0, 0] and viol.dtype == np.int32
    assert keep.tolist() == [0, 0, 1, 0] and keep.dtype == np.uint8     # the row beyond the count: 0 and 0
    assert cr.free_space(P, 3, depths, poses, K, 0.05, 1, 3)[1].tolist() == [0, 1, 1, 0]
    assert cr.free_space(P, 3, depths, poses, K, 0.05, 1, 4)[1].tolist() == [1, 1, 1, 0]
    assert cr.free_space(P, 0, depths, poses, K)[0].tolist() == [0, 0, 0, 0]


def test_ref_uses_the_pose():
    # the camera moved 1 m forward: the point at world z = 2 is 1 m in front of it
    T = EYE.copy()
    T[2, 3] = 1.0
    P = np.array([[0, 0, 2.0]], f32)
    D = np.full((H, W), 1.5, f32)
    assert cr.violates(P, D, T, K, 0.05, 1).tolist() == [True]
    assert cr.violates(P, D, EYE, K, 0.05, 1).tolist() == [False]


# ------------------------------------------------------------------------------------------ the demonstration
# measured with the oracle loop (ground-truth poses) and the restated carve after every step, margin 0.05, window 1:
#   scene    rows without -> with   ghost rows in the last view   RMSE of the last model view against its frame
DEMO = {"wave": (11817, 11106, 680, 0.11983047251575103, 0.0040628909924559165),
        "facets": (11873, 11168, 673, 0.11868185921789236, 0.002756892772858467)}


def _loop(s, margin=None, window=1):
    Kc = s["intrinsics"][0]
    removed = []

    def per_frame(i, m, pose):
        removed.append(cr.carve_map(m, s["depths"][i], pose, Kc, margin, window))

    m, poses = oslam.run_sequence(s["colors"], s["depths"], Kc, s["poses"], odom="gt",
                                  per_frame=None if margin is None else per_frame)
    r = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[-1], Kc, cr.SEQ_H, cr.SEQ_W)
    st = rr.residual_stats(r.depth, s["depths"][-1])
    return m, removed, cr.ghost_rows(m.points, s["clean"][-1], poses[-1], Kc), st


@pytest.mark.parametrize("scene", ["wave", "facets"])
def test_carving_removes_the_ghost_of_a_block_that_moved_away(scene):
    s = cr.block_sequence(scene, moved=True)
    rows0, rows1, ghosts0, rmse0, rmse1 = DEMO[scene]
    plain, _, ghosts, st = _loop(s)
    print(scene, "without carving: rows", len(plain), "ghost rows", ghosts, "rmse", st["rmse"], "coverage", st["coverage"])
    assert (len(plain), ghosts) == (rows0, ghosts0)
    assert st["rmse"] == pytest.approx(rmse0, rel=1e-9) and st["coverage"] == 1.0
    carved, removed, ghosts, st = _loop(s, 0.05, 1)
    print(scene, "with carving: rows", len(carved), "ghost rows", ghosts, "rmse", st["rmse"], "removed per step", removed)
    assert (len(carved), ghosts) == (rows1, 0)
    assert st["rmse"] == pytest.approx(rmse1, rel=1e-9) and st["coverage"] == 1.0
    # nothing goes while the block stands still in front of the same background (steps 0..4: the frame of step 5 is
    # the last one that shows it); the bulk goes with the first frame that sees through it
    assert removed[:5] == [0] * 5 and removed[6] > 600 and sum(removed[9:]) == 0
    # window 0 would take silhouette rows of the block while it is still there: that is why the window exists
    _, removed0, _, _ = _loop(s, 0.05, 0)
    assert sum(removed0[:5]) > 0


@pytest.mark.parametrize("scene", ["wave", "facets"])
def test_carving_removes_nothing_from_an_undisturbed_sequence(scene):
    """the condition that keeps the demonstration honest"""
    s = cr.block_sequence(scene, moved=False)
    plain, _, ghosts, st = _loop(s)
    carved, removed, _, st1 = _loop(s, 0.05, 1)
    assert removed == [0] * cr.SEQ_L
    assert ghosts == 0 and len(carved) == len(plain) and st1 == st
    assert np.array_equal(carved.points, plain.points) and np.array_equal(carved.ccounts, plain.ccounts)


# ------------------------------------------------------------------------------------------ the C entry point
def _seq(**kw):
    """a descriptor that passes every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and
    every case below is rejected before one)"""
    d = dict(points=0x1000, n_bound=100, n_dev=0, depth=0x2000, depth_stride_view=48 * 64, poses16=0x3000, K16=0x4000,
             violations=0x5000, keep=0x6000)
    d.update(kw)
    return d


def _fill(q, d):
    q.map = _C.MapView(d["points"], 0, 0, 0, d["n_bound"], d["n_bound"], d["n_dev"])
    for k in ("depth", "depth_stride_view", "poses16", "K16", "violations", "keep"):
        setattr(q, k, d[k])


ARGS = dict(B=1, L=2, H=48, W=64, margin=0.05, window=1, min_views=1)
INVALID = {
    "null_points": (dict(points=0), {}, "NULL"),
    "null_depth": (dict(depth=0), {}, "NULL"),
    "null_poses": (dict(poses16=0), {}, "NULL"),
    "null_K": (dict(K16=0), {}, "NULL"),
    "null_both_outputs": (dict(violations=0, keep=0), {}, "NULL"),
    "negative_bound": (dict(n_bound=-1), {}, "n_bound"),
    "no_sequences": ({}, dict(B=0), "bad arguments"),
    "no_views": ({}, dict(L=0), "bad arguments"),
    "no_rows_of_pixels": ({}, dict(H=0), "bad arguments"),
    "negative_width": ({}, dict(W=-3), "bad arguments"),
    "too_many_pixels": ({}, dict(H=1 << 16, W=1 << 15), "too large"),
    "negative_margin": ({}, dict(margin=-0.01), "margin"),
    "nan_margin": ({}, dict(margin=NAN), "margin"),
    "infinite_margin": ({}, dict(margin=float("inf")), "margin"),
    "negative_window": ({}, dict(window=-1), "window"),
    "wide_window": ({}, dict(window=4), "window"),
    "zero_min_views": ({}, dict(min_views=0), "min_views"),
}


def _call(lib, seqs, a):
    return lib.gs_free_space_dc_f32(seqs, a["B"], a["L"], a["H"], a["W"], a["margin"], a["window"], a["min_views"], None)


@pytest.mark.parametrize("case", sorted(INVALID))
def test_entry_point_rejects_before_any_hip_call(case):
    lib = _C.lib()
    change, args, word = INVALID[case]
    seqs = (_C.CarveSeq * 1)()
    _fill(seqs[0], _seq(**change))
    assert _call(lib, seqs, dict(ARGS, **args)) == 1       # GS_ERR_INVALID
    assert word in lib.gs_last_error().decode(), lib.gs_last_error()


def test_entry_point_checks_every_sequence_and_the_descriptor_pointer():
    lib = _C.lib()
    seqs = (_C.CarveSeq * 2)()
    for q in seqs:
        _fill(q, _seq())
    assert _call(lib, None, ARGS) == 1
    _fill(seqs[1], _seq(depth=0))
    assert _call(lib, seqs, dict(ARGS, B=2)) == 1
    assert "NULL" in lib.gs_last_error().decode()


def test_symbol_is_exported_and_the_abi_version_stays():
    assert "gs_free_space_dc_f32" in _C.EXPORTS
    assert _C.ABI_VERSION == 3 and _C.lib().gs_abi_version() == 3
    assert hasattr(_C.lib(), "gs_free_space_dc_f32")
    hdr = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    assert "gs_free_space_dc_f32" in hdr and "typedef struct gs_carve_seq" in hdr


def test_carve_kernel_uses_no_scratch_and_spills_nothing():
    """a gather-bound pass over the map: a spill would add private-segment traffic to every row, and 8 waves per SIMD
    (<= 64 VGPRs) keep enough gathers in flight"""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_carve.hip", "gs_free_space_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_free_space_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_free_space_kernel"}, r.stdout
    vgpr, sgpr, scratch, occ, sspill, vspill, lds = rows["gs_free_space_kernel"]
    assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (scratch, vspill, sspill)
    assert int(vgpr) <= 64 and int(occ) >= 8, (vgpr, occ)
    assert int(lds) == 16 * 96, lds      # 16 cameras


# ------------------------------------------------------------------------------------------ ops arguments
def _ops_inputs(B=1, L=2, n=5):
    maps = [(torch.zeros(n, 3), None, None, None, None, None) for _ in range(B)]
    return maps, torch.ones(B, L, H, W), torch.eye(4).expand(B, L, 4, 4), torch.eye(4).expand(B, 4, 4)


def test_ops_have_no_cpu_fallback():
    from gradslam_amd import ops
    maps, depth, poses, Kt = _ops_inputs()
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.free_space_batch(maps, depth, poses, Kt)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.free_space_batch(maps, depth.unsqueeze(-1), poses, Kt, margin=0, window=0, min_views=2)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.free_space(torch.zeros(5, 3), depth[0], poses[0], Kt[0])
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.free_space(torch.zeros(5, 3), depth[0, 0], poses[0, 0], Kt[0])


def test_ops_argument_errors_name_the_argument():
    from gradslam_amd import ops
    maps, depth, poses, Kt = _ops_inputs()
    for kw, exc, word in ((dict(margin="0.05"), TypeError, "margin"), (dict(margin=True), TypeError, "margin"),
                          (dict(margin=-1.0), ValueError, "margin"), (dict(margin=NAN), ValueError, "margin"),
                          (dict(margin=float("inf")), ValueError, "margin"), (dict(window=1.0), TypeError, "window"),
                          (dict(window=-1), ValueError, "window"), (dict(window=4), ValueError, "window"),
                          (dict(min_views=0), ValueError, "min_views"), (dict(min_views=1.5), TypeError, "min_views")):
        with pytest.raises(exc, match=word):
            ops.free_space_batch(maps, depth, poses, Kt, **kw)
        with pytest.raises(exc, match=word):
            ops.free_space(maps[0][0], depth[0], poses[0], Kt[0], **kw)
    with pytest.raises(TypeError, match="depth"):
        ops.free_space_batch(maps, depth.numpy(), poses, Kt)
    with pytest.raises(TypeError, match="poses"):
        ops.free_space_batch(maps, depth, None, Kt)
    with pytest.raises(TypeError, match="K"):
        ops.free_space(maps[0][0], depth[0], poses[0], K)
    with pytest.raises(ValueError, match="maps"):
        ops.free_space_batch([], depth, poses, Kt)
    with pytest.raises(ValueError, match="depth"):
        ops.free_space_batch(maps, depth[0], poses, Kt)
    with pytest.raises(ValueError, match="depth"):
        ops.free_space_batch(maps + maps, depth, poses, Kt)
    with pytest.raises(ValueError, match="depth"):
        ops.free_space_batch(maps, torch.ones(1, 2, H, W, 3), poses, Kt)
    with pytest.raises(ValueError, match="poses"):
        ops.free_space_batch(maps, depth, poses[:, :1], Kt)
    with pytest.raises(ValueError, match="K"):
        ops.free_space_batch(maps, depth, poses, Kt[0])
    with pytest.raises(ValueError, match="points"):
        ops.free_space_batch([(torch.zeros(5, 4), None, None, None, None, None)], depth, poses, Kt)
    with pytest.raises(ValueError, match="out"):
        ops.free_space_batch(maps, depth, poses, Kt, out=([torch.zeros(5, dtype=torch.int32)],))


# ------------------------------------------------------------------------------------------ Pointclouds arguments
def _frames(B=1, L=1, poses=True):
    return RGBDImages(torch.zeros(B, L, H, W, 3), torch.ones(B, L, H, W, 1), torch.from_numpy(K).expand(B, 1, 4, 4),
                      torch.eye(4).expand(B, L, 4, 4) if poses else None)


def _cpu_map(B=1, n=6):
    g = torch.Generator().manual_seed(0)
    mk = lambda c: [torch.rand(n, c, generator=g) for _ in range(B)]   # noqa: E731
    return Pointclouds(mk(3), mk(3), mk(3), mk(1))


@pytest.mark.parametrize("method", ["carve_", "carve", "free_space_violations"])
def test_pointclouds_carve_argument_errors(method):
    pc = _cpu_map()
    with pytest.raises(ValueError, match="empty"):
        getattr(Pointclouds(), method)(_frames())
    with pytest.raises(TypeError, match="RGBDImages"):
        getattr(pc, method)(torch.ones(1, 1, H, W))
    with pytest.raises(ValueError, match="poses"):
        getattr(pc, method)(_frames(poses=False))
    with pytest.raises(ValueError, match="one sequence per pointcloud"):
        getattr(pc, method)(_frames(B=2))
    with pytest.raises(ValueError, match="margin"):
        getattr(pc, method)(_frames(), margin=-0.1)
    with pytest.raises(TypeError, match="window"):
        getattr(pc, method)(_frames(), window="1")
    with pytest.raises(ValueError, match="window"):
        getattr(pc, method)(_frames(), window=4)
    if method != "free_space_violations":
        with pytest.raises(ValueError, match="min_views"):
            getattr(pc, method)(_frames(), min_views=0)
    # a CPU map has no kernel to run: it says so instead of computing with torch
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        getattr(pc, method)(_frames())
    assert pc._n == [6] and pc.last_pruned is None


# ------------------------------------------------------------------------------------------ PointFusion arguments
def test_pointfusion_carve_arguments():
    slam = PointFusion()
    assert slam.carve_margin is None and slam.carve_window == 1 and slam.carve_every == 1
    slam = PointFusion(carve_margin=0.02, carve_window=2, carve_every=3)
    assert (slam.carve_margin, slam.carve_window, slam.carve_every) == (0.02, 2, 3)
    assert PointFusion(carve_margin=0).carve_margin == 0
    for kw in (dict(carve_margin="0.1"), dict(carve_margin=True), dict(carve_margin=0.1, carve_window=1.0),
               dict(carve_margin=0.1, carve_every=None), dict(carve_window=False)):
        with pytest.raises(TypeError):
            PointFusion(**kw)
    for kw in (dict(carve_margin=-0.1), dict(carve_margin=NAN), dict(carve_margin=float("inf")),
               dict(carve_margin=0.1, carve_window=-1), dict(carve_margin=0.1, carve_window=4),
               dict(carve_margin=0.1, carve_every=0), dict(carve_every=0)):
        with pytest.raises(ValueError):
            PointFusion(**kw)
    from gradslam_amd.slam.icpslam import ICPSLAM
    with pytest.raises(TypeError):
        ICPSLAM(carve_margin=0.05)       # like pruning, carving is a map-fusion feature


class _CountingMap(Pointclouds):
    calls = None

    def mark_epoch(self):
        self.calls.append("mark")
        return super().mark_epoch()

    def prune_(self, *a, **kw):
        self.calls.append("prune")
        return super().prune_(*a, **kw)

    def carve_(self, frames, **kw):
        # (no GPU here: the schedule and the arguments of the call, not the kernel)
        self.calls.append(("carve", frames, kw))
        return self


class _NoKernels(PointFusion):
    """the schedule around a step without the kernels of the step: the step itself appends two rows"""

    def _localize(self, pointclouds, live_frame, prev_frame):
        return torch.eye(4).view(1, 1, 4, 4) * 1.0

    def _map(self, pointclouds, live_frame, inplace=False):
        new = type(pointclouds)(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2, 3),
                                torch.tensor([[[0.0], [1.0]]]))
        return pointclouds.append_points(new)


def _fake_frame():
    return RGBDImages(torch.zeros(1, 1, 2, 2, 3), torch.ones(1, 1, 2, 2, 1), torch.eye(4).view(1, 1, 4, 4),
                      torch.eye(4).view(1, 1, 4, 4))


def test_default_step_never_carves():
    pc = _CountingMap()
    pc.calls = []
    slam = _NoKernels(odom="gt")
    for _ in range(5):
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=True)
    assert pc.calls == [] and pc._carve_steps == 0


def test_carving_step_schedule_and_arguments():
    pc = _CountingMap()
    pc.calls = []
    slam = _NoKernels(odom="gt", carve_margin=0.03, carve_window=2, carve_every=2, prune_min_confidence=0.5,
                      prune_min_age=1, prune_every=4)
    frames = []
    for _ in range(4):
        frames.append(_fake_frame())
        pc, _ = slam.step(pc, frames[-1], None, inplace=True)
    kinds = [c if isinstance(c, str) else c[0] for c in pc.calls]
    # the carve of a step comes after its map update and before its pruning schedule
    assert kinds == ["mark", "carve", "mark", "mark", "carve", "prune", "mark"]
    carves = [c for c in pc.calls if not isinstance(c, str)]
    assert len(carves) == 2 and carves[0][1] is frames[1] and carves[1][1] is frames[3]   # the frame just fused
    assert all(c[2] == dict(margin=0.03, window=2, min_views=1) for c in carves)
    assert all(c[1].poses is not None and c[1].shape[1] == 1 for c in carves)
    assert pc._carve_steps == 4
    assert pc.clone()._carve_steps == 4


class _FirstRowCarver(Pointclouds):
    """a CPU map whose carve removes its oldest row through prune_(keep=...), as carve_ does with the kernel's mask"""

    def carve_(self, frames, **kw):
        keep = torch.ones(self._n[0], dtype=torch.bool)
        keep[0] = False
        return self.prune_(None, keep=[keep])


class _TwoRowsAStep(PointFusion):
    """a step that appends a row of confidence 0 and a row of confidence 1, both with x = the step number; out of place
    it returns a fresh container, as the map update does: no marks, the step counters at 0"""
    steps = 0

    def _localize(self, pointclouds, live_frame, prev_frame):
        return torch.eye(4).view(1, 1, 4, 4) * 1.0

    def _map(self, pointclouds, live_frame, inplace=False):
        self.steps += 1
        x = torch.full((1, 2, 3), float(self.steps))
        new = type(pointclouds)(x, torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.tensor([[[0.0], [1.0]]]))
        if inplace:
            return pointclouds.append_points(new)
        out = type(pointclouds)()
        if pointclouds.has_points:
            out.append_points(pointclouds)
        return out.append_points(new)


@pytest.mark.parametrize("inplace", [True, False])
def test_carve_then_prune_step_reads_the_rewritten_marks(inplace):
    """carve + prune in one step: the pruning schedule reads the marks that the carve's compaction rewrote, in place and
    out of place (there the new container takes the marks once, before the carve).  Expected, restated on lists: a step
    appends (step, 0.0), (step, 1.0); the carve drops row 0 and lowers every mark by the rows dropped in front of it; the
    prune (every step, min_age 1) drops rows below 0.5 in front of the newest mark and rewrites the marks; then the count
    is the new mark.  The confidence-0 row of a step sits exactly at the true newest mark: a mark left one too high
    prunes it a step early."""
    slam = _TwoRowsAStep(odom="gt", carve_margin=0.05, prune_min_confidence=0.5, prune_min_age=1, prune_every=1)
    pc = _FirstRowCarver()
    rows, marks = [], []
    for step in range(1, 7):
        before = pc
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=inplace)
        assert (pc is before) == inplace and type(pc) is _FirstRowCarver
        rows += [(float(step), 0.0), (float(step), 1.0)]
        rows, marks = rows[1:], [max(m - 1, 0) for m in marks]                        # the carve
        if marks:                                                                     # the prune
            s = [c >= 0.5 or i >= marks[-1] for i, (_, c) in enumerate(rows)]
            marks = [sum(s[:m]) for m in marks]
            rows = [r for r, k in zip(rows, s) if k]
        marks.append(len(rows))                                                       # the epoch
        got = list(zip(pc.points_list[0][:, 0].tolist(), pc.features_list[0][:, 0].tolist()))
        assert got == rows, (step, got, rows)
        assert pc._marks[0, :pc._n_marks].tolist() == marks, (step, pc._marks[0, :pc._n_marks].tolist(), marks)
        assert pc._carve_steps == pc._prune_steps == step
    assert (float(step), 0.0) in rows and (float(step - 1), 0.0) not in rows   # (the young row is there, the older one went)
