"""CPU tests of the bilateral depth filter: the NumPy restatement (tests/bilateral_ref.py) and its float64 adjoint, the
argument checks of the two C entry points (made before any HIP call, so they run without a GPU), the register report of
the two kernels (cross-compiled) and the argument checks of the Python layers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from oracle import oracle
from tests import backward_cases as bc
from tests import bilateral_ref as br

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("H,W", br.SIZES)
def test_ref_radius_zero_is_the_identity_in_bits(H, W):
    d = br.case(H, W)
    out, wsum = br.bilateral(d, radius=0)
    assert np.array_equal(br.bits(out), br.bits(d))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(wsum, (d > 0).astype(np.float32))


@pytest.mark.parametrize("radius", br.RADII)
@pytest.mark.parametrize("H,W", br.SIZES)
def test_ref_keeps_the_valid_mask_and_normaliser_at_least_one(H, W, radius):
    d = br.case(H, W)
    out, wsum = br.bilateral(d, radius=radius)
    with np.errstate(invalid="ignore"):
        valid = d > 0
        assert np.array_equal(out > 0, valid)
    assert (wsum[valid] >= 1.0).all() and (wsum[~valid] == 0.0).all()
    assert np.array_equal(br.bits(out)[~valid], br.bits(d)[~valid])     # invalid centres are copied through, NaN included
    assert out[valid].min() >= d[valid].min() and out[valid].max() <= d[valid].max()   # a convex combination


def test_case_holds_what_the_tests_say_it_holds():
    d = br.case(67, 131)
    with np.errstate(invalid="ignore"):
        valid = d > 0
        assert np.isnan(d).sum() == 1 and (d < 0).sum() == 1 and (d[:, -1] == 0).all() and (d[-1] == 0).all()
    assert 0.02 < 1 - valid[:-1, :-1].mean() < 0.1                                     # holes
    jumps = np.abs(np.diff(d, axis=1))[valid[:, 1:] & valid[:, :-1]]
    assert jumps.max() > 0.7                                                           # the step
    assert (br.case(1, 1) > 0).all() and (br.case(2, 2) > 0).any()
    assert not br.case(9, 65).flags.writeable


def test_ref_does_not_smear_the_step():
    """sigma_range 0.03 m against a 0.8 m step: a weight across the step is exp(-0.64 / 0.0018) = 0 in float32, so the
    two sides never mix"""
    clean, noisy, _ = br.plane_scene()
    out, _ = br.bilateral(noisy, **br.DEFAULTS)
    left = np.zeros_like(noisy, dtype=bool)
    left[:, :noisy.shape[1] // 2] = True
    valid = noisy > 0
    assert out[valid & left].max() < noisy[valid & ~left].min()
    assert out[valid & left].max() <= noisy[valid & left].max() and out[valid & ~left].min() >= noisy[valid & ~left].min()


def _mean_normal_error_deg(depth, clean, K):
    _, n, _, valid = oracle.frame_maps(depth, K)
    _, n0, _, _ = oracle.frame_maps(clean, K)
    ok = valid & (np.linalg.norm(n, axis=-1) > 0) & (np.linalg.norm(n0, axis=-1) > 0)
    cos = np.clip((n[ok].astype(np.float64) * n0[ok]).sum(-1), -1.0, 1.0)
    return float(np.degrees(np.arccos(cos)).mean()), ok


def test_ref_lowers_the_normal_error_of_the_noisy_plane():
    """48 x 64 inclined plane with a 0.8 m step, fx = 60, 4 mm noise, 5 % holes: the frame normals of the filtered depth
    are closer to those of the clean depth than the normals of the raw depth (same pixels: the mask is unchanged)"""
    clean, noisy, K = br.plane_scene()
    out, _ = br.bilateral(noisy, **br.DEFAULTS)
    assert np.array_equal(out > 0, noisy > 0)
    raw, ok_raw = _mean_normal_error_deg(noisy, clean, K)
    fil, ok_fil = _mean_normal_error_deg(out, clean, K)
    valid = noisy > 0
    rmse = lambda a: float(np.sqrt(((a[valid].astype(np.float64) - clean[valid]) ** 2).mean()))   # noqa: E731
    print("mean normal error: raw %.2f deg, filtered %.2f deg; depth rmse raw %.2f mm, filtered %.2f mm"
          % (raw, fil, 1e3 * rmse(noisy), 1e3 * rmse(out)))
    assert np.array_equal(ok_raw, ok_fil)
    assert fil < raw
    assert rmse(out) < rmse(noisy)


# ------------------------------------------------------------------------------------------ the adjoint
@pytest.mark.parametrize("H,W,radius", [(2, 2, 1), (9, 65, 1), (9, 65, 3), (67, 131, 8)])
def test_float64_adjoint_agrees_with_central_differences(H, W, radius):
    d = br.case(H, W).astype(np.float64)
    ob = br.weights(H, W).astype(np.float64)
    kw = dict(br.DEFAULTS, radius=radius)
    bar = br.adjoint(d, ob, **kw)
    with np.errstate(invalid="ignore"):
        valid = d > 0
    assert np.array_equal(bar[~valid], ob[~valid])
    rng = np.random.default_rng([3, H, W, radius])
    picks = np.argwhere(valid)
    picks = picks[rng.choice(len(picks), size=min(12, len(picks)), replace=False)]
    h = 1e-6

    def loss(x):
        out, _ = br.forward_np(x, **kw)
        return float((np.where(valid, out, 0.0) * ob).sum())

    scale = np.abs(bar[valid]).max()
    for y, x in picks:
        dp, dm = d.copy(), d.copy()
        dp[y, x] += h
        dm[y, x] -= h
        fd = (loss(dp) - loss(dm)) / (2 * h)
        # central differences of a smooth function: truncation ~ h^2 f''' (f''' <~ 1 / sigma_range^3 = 4e4 -> 4e-8),
        # cancellation ~ eps64 * |loss| / h ~ 1e-16 * 1e3 / 1e-6 = 1e-7
        assert abs(fd - bar[y, x]) <= 1e-6 * scale, (y, x, fd, bar[y, x])


@pytest.mark.parametrize("H,W,radius", br.BACKWARD_CASES)
def test_committed_gap_has_not_drifted(H, W, radius):
    want = br.BACKWARD_GAP[br.backward_key(H, W, radius)]
    got = br.backward_gap(H, W, radius)
    assert want / bc.DRIFT <= got <= want * bc.DRIFT, (got, want)


def test_adjoint_is_zero_where_no_upstream_reaches():
    H, W, r = 20, 70, 3
    d = br.case(H, W)
    ob = np.zeros((H, W), np.float32)
    ob[:6, :9] = br.weights(H, W)[:6, :9]
    bar = br.adjoint(d, ob, radius=r)
    assert (bar[6 + r:, :] == 0).all() and (bar[:, 9 + r:] == 0).all() and np.abs(bar[:6, :9]).max() > 0


# ------------------------------------------------------------------------------------------ the C entry points
def _fwd(**kw):
    """arguments that pass every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and every case
    below is rejected before one)"""
    a = dict(depth=0x100000, stride_frame=48 * 64, stride_row=64, n=2, H=48, W=64, radius=3, two_s=8.0, two_r=0.0018,
             out=0x200000, wsum=0x300000)
    a.update(kw)
    return [a[k] for k in ("depth", "stride_frame", "stride_row", "n", "H", "W", "radius", "two_s", "two_r", "out",
                           "wsum")] + [None]


def _bwd(**kw):
    a = dict(depth=0x100000, stride_frame=48 * 64, stride_row=64, out=0x200000, wsum=0x300000, out_bar=0x400000, n=2,
             H=48, W=64, radius=3, two_s=8.0, two_r=0.0018, depth_bar=0x500000)
    a.update(kw)
    return [a[k] for k in ("depth", "stride_frame", "stride_row", "out", "wsum", "out_bar", "n", "H", "W", "radius",
                           "two_s", "two_r", "depth_bar")] + [None]


INVALID_FWD = {
    "null_depth": (dict(depth=0), "NULL"),
    "null_out": (dict(out=0), "NULL"),
    "radius_9": (dict(radius=9), "radius"),
    "radius_negative": (dict(radius=-1), "radius"),
    "sigma_space_zero": (dict(two_s=0.0), "sigma"),
    "sigma_range_negative": (dict(two_r=-0.0018), "sigma"),
    "sigma_range_nan": (dict(two_r=float("nan")), "sigma"),
    "sigma_space_inf": (dict(two_s=float("inf")), "sigma"),
    "alias_out": (dict(out=0x100000), "alias"),
    "alias_out_second_frame": (dict(out=0x100000 + 4 * 48 * 64), "alias"),
    "alias_wsum": (dict(wsum=0x100000), "alias"),
    "alias_wsum_out": (dict(wsum=0x200000), "alias"),
    "row_stride": (dict(stride_row=63), "stride"),
    "frame_stride": (dict(stride_frame=100), "stride"),
    "no_frames": (dict(n=0), "positive"),
    "empty_image": (dict(W=0), "positive"),
}
INVALID_BWD = {
    "null_wsum": (dict(wsum=0), "NULL"),
    "null_out_bar": (dict(out_bar=0), "NULL"),
    "null_depth_bar": (dict(depth_bar=0), "NULL"),
    "radius_9": (dict(radius=9), "radius"),
    "sigma_range_zero": (dict(two_r=0.0), "sigma"),
    "alias_out_bar": (dict(depth_bar=0x400000), "alias"),
    "alias_depth": (dict(depth_bar=0x100000), "alias"),
}


@pytest.mark.parametrize("case", sorted(INVALID_FWD))
def test_forward_entry_point_rejects_before_any_hip_call(case):
    lib = _C.lib()
    change, word = INVALID_FWD[case]
    assert lib.gs_bilateral_depth_f32(*_fwd(**change)) == 1       # GS_ERR_INVALID
    msg = lib.gs_last_error().decode()
    assert msg.startswith("gs_bilateral_depth_f32") and word in msg, msg


@pytest.mark.parametrize("case", sorted(INVALID_BWD))
def test_backward_entry_point_rejects_before_any_hip_call(case):
    lib = _C.lib()
    change, word = INVALID_BWD[case]
    assert lib.gs_bilateral_depth_backward_f32(*_bwd(**change)) == 1
    msg = lib.gs_last_error().decode()
    assert msg.startswith("gs_bilateral_depth_backward_f32") and word in msg, msg


def test_exports_are_bound():
    assert {"gs_bilateral_depth_f32", "gs_bilateral_depth_backward_f32"} <= set(_C.EXPORTS)


def test_bilateral_kernels_use_no_scratch_and_spill_nothing():
    """Each thread walks its window out of LDS with a handful of registers: no private segment, no spill; the forward
    keeps 8 waves per SIMD, the backward (31 KB of LDS per block) at least 4."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_bilateral.hip",
                        "gs_bilateral_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_bilateral_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_bilateral_depth_kernel", "gs_bilateral_depth_backward_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
    assert int(rows["gs_bilateral_depth_kernel"][0]) <= 64 and int(rows["gs_bilateral_depth_kernel"][3]) >= 8
    assert int(rows["gs_bilateral_depth_kernel"][6]) <= 8 * 1024 + 4 * 289
    assert int(rows["gs_bilateral_depth_backward_kernel"][3]) >= 4


# ------------------------------------------------------------------------------------------ the Python layers
def test_ops_have_no_cpu_fallback():
    from gradslam_amd import ops
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.bilateral_depth(torch.ones(4, 5))
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.bilateral_depth(torch.ones(2, 4, 5, requires_grad=True))
    from gradslam_amd.structures.rgbdimages import RGBDImages
    fr = RGBDImages(torch.zeros(1, 1, 4, 5, 3), torch.ones(1, 1, 4, 5, 1), torch.eye(4).view(1, 1, 4, 4))
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        fr.bilateral_filter()


def test_ops_argument_errors():
    from gradslam_amd import ops
    d = torch.ones(4, 5)
    for bad in (9, -1):
        with pytest.raises(ValueError, match="radius"):
            ops.bilateral_depth(d, radius=bad)
    for bad in (2.0, True, "3"):
        with pytest.raises(TypeError, match="radius"):
            ops.bilateral_depth(d, radius=bad)
    for name in ("sigma_space", "sigma_range"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                ops.bilateral_depth(d, **{name: bad})
        with pytest.raises(TypeError, match=name):
            ops.bilateral_depth(d, **{name: "1"})
    with pytest.raises(ValueError, match="H, W"):
        ops.bilateral_depth(torch.ones(5))


def test_slam_depth_filter_arguments():
    from gradslam_amd.slam.icpslam import ICPSLAM
    from gradslam_amd.slam.pointfusion import PointFusion
    for cls in (ICPSLAM, PointFusion):
        assert cls(odom="gt").depth_filter is None
        assert cls(odom="gt", depth_filter={}).depth_filter == dict(radius=3, sigma_space=2.0, sigma_range=0.03)
        assert cls(odom="gt", depth_filter=dict(radius=0, sigma_range=1)).depth_filter == \
            dict(radius=0, sigma_space=2.0, sigma_range=1)
        with pytest.raises(TypeError, match="depth_filter"):
            cls(odom="gt", depth_filter=3)
        with pytest.raises(TypeError, match="radius"):
            cls(odom="gt", depth_filter=dict(radius=2.0))
        with pytest.raises(TypeError, match="radius"):
            cls(odom="gt", depth_filter=dict(radius=True))
        with pytest.raises(ValueError, match="radius"):
            cls(odom="gt", depth_filter=dict(radius=9))
        with pytest.raises(TypeError, match="sigma_space"):
            cls(odom="gt", depth_filter=dict(sigma_space="2"))
        with pytest.raises(ValueError, match="sigma_range"):
            cls(odom="gt", depth_filter=dict(sigma_range=0))
        with pytest.raises(ValueError, match="sigma_space"):
            cls(odom="gt", depth_filter=dict(sigma_space=float("nan")))
        with pytest.raises(ValueError, match="unknown"):
            cls(odom="gt", depth_filter=dict(sigma=1.0))


class _Recorder(object):
    """stands in for the kernels of a step: records which frame each stage was handed"""

    def __init__(self):
        self.seen = []


def _slam_without_kernels(cls, rec, **kw):
    class NoKernels(cls):
        def _filtered(self, live_frame):
            if self.depth_filter is None:
                return live_frame
            rec.seen.append(("filter", dict(self.depth_filter)))
            other = live_frame[:, :]            # a new container sharing every tensor
            other._tag = "filtered"
            return other

        def _localize(self, pointclouds, live_frame, prev_frame):
            rec.seen.append(("localize", getattr(live_frame, "_tag", "raw")))
            return torch.full((1, 1, 4, 4), 7.0)

        def _map(self, pointclouds, live_frame, inplace=False):
            rec.seen.append(("map", getattr(live_frame, "_tag", "raw")))
            return pointclouds
    return NoKernels(odom="gt", **kw)


def _frame():
    from gradslam_amd.structures.rgbdimages import RGBDImages
    return RGBDImages(torch.zeros(1, 1, 2, 2, 3), torch.ones(1, 1, 2, 2, 1), torch.eye(4).view(1, 1, 4, 4),
                      torch.eye(4).view(1, 1, 4, 4))


@pytest.mark.parametrize("which", ["ICPSLAM", "PointFusion"])
def test_step_works_on_the_filtered_copy_and_writes_the_pose_back(which):
    from gradslam_amd import slam as S
    from gradslam_amd.structures.pointclouds import Pointclouds
    cls = getattr(S, which)
    rec = _Recorder()
    slam = _slam_without_kernels(cls, rec, depth_filter=dict(radius=2))
    live = _frame()
    pc, poses = slam.step(Pointclouds(), live, None, inplace=True)
    assert rec.seen == [("filter", dict(radius=2, sigma_space=2.0, sigma_range=0.03)), ("localize", "filtered"),
                        ("map", "filtered")]
    assert float(poses[0, 0, 0, 0]) == 7.0 and live.poses is poses       # the caller's frame has the recovered pose
    rec = _Recorder()
    slam = _slam_without_kernels(cls, rec)
    live = _frame()
    pc, poses = slam.step(Pointclouds(), live, None, inplace=True)
    assert rec.seen == [("localize", "raw"), ("map", "raw")] and live.poses is poses   # no new call with None
    with pytest.raises(TypeError, match="live_frame"):
        _slam_without_kernels(cls, _Recorder(), depth_filter={}).step(Pointclouds(), "frame", None)
