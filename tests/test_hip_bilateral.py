"""GPU tests of the bilateral depth filter (gs_bilateral.hip -> gs_bilateral_depth_f32 / _backward_f32 ->
ops.bilateral_depth -> RGBDImages.bilateral_filter -> ICPSLAM / PointFusion(depth_filter=...)).

Forward and wsum: EQUAL BITS against the NumPy restatement (tests/bilateral_ref.py), no tolerance.  Backward: against the
float64 adjoint within backward_cases.kernel_bound(committed float32-vs-float64 gap of the case).  Drivers: equal bits
against the same driver fed pre-filtered frames.  Tile = 64 x 8 pixels, halo = radius: the sizes sit at one pixel, one
block, one row / column of tiles, odd sizes over several tiles and the tile exceeded by one pixel in each direction; radius 8
is wider than the small images."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from tests import backward_cases as bc
from tests import bilateral_ref as br

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def dev(a):
    return T(np.array(a, copy=True, order="C")).cuda()      # (a copy: the cases are read-only arrays)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gs():
    assert torch.cuda.is_available()
    import gradslam_amd
    return gradslam_amd


_REF = {}


def ref(H, W, radius, seed=0):
    """(out, wsum) of the restatement on the case, computed once and never changed"""
    key = (H, W, radius, seed)
    if key not in _REF:
        _REF[key] = br.bilateral(br.case(H, W, seed), **dict(br.DEFAULTS, radius=radius))
    return _REF[key]


def same_bits(got, want, what):
    got, want = br.bits(host(got)), br.bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d words differ" % (what, (got != want).sum(), got.size)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("radius", br.RADII)
@pytest.mark.parametrize("H,W", br.SIZES)
def test_forward_and_wsum_equal_the_restatement(ops, H, W, radius):
    """holes, a negative and a NaN centre, an invalid last column and last row and the 0.8 m step are part of every
    case that has room for them (bilateral_ref.case)"""
    d = br.case(H, W)
    out, wsum = ops.bilateral_depth(dev(d), return_wsum=True, **dict(br.DEFAULTS, radius=radius))
    want_out, want_w = ref(H, W, radius)
    same_bits(out, want_out, "out")
    same_bits(wsum, want_w, "wsum")
    if radius == 0:
        same_bits(out, d, "radius 0 is the identity")
    only = ops.bilateral_depth(dev(d), **dict(br.DEFAULTS, radius=radius))      # (the launch without wsum)
    same_bits(only, want_out, "out without wsum")


def test_other_sigmas(ops):
    d = br.case(67, 131)
    kw = dict(radius=2, sigma_space=0.7, sigma_range=0.4)      # (a range sigma that mixes across holes' neighbours)
    out, wsum = ops.bilateral_depth(dev(d), return_wsum=True, **kw)
    want = br.bilateral(d, **kw)
    same_bits(out, want[0], "out")
    same_bits(wsum, want[1], "wsum")


def test_strided_slice_of_a_longer_stack_is_read_in_place(ops):
    """3 frames taken as every second frame of a stack of 7, and a column crop of a wider stack: per-frame and per-row
    strides; `out=` receives the result"""
    H, W = 9, 65
    stack = np.stack([br.case(H, W, seed=s) for s in range(7)])
    big = dev(stack)
    sl = big[1:7:2]
    assert not sl.is_contiguous()
    out = torch.full((3, H, W), -7.0, device="cuda")
    res, wsum = ops.bilateral_depth(sl, out=out, return_wsum=True, **br.DEFAULTS)
    assert res is out
    for i, s in enumerate((1, 3, 5)):
        want = ref(H, W, 3, seed=s)
        same_bits(out[i], want[0], "frame %d" % s)
        same_bits(wsum[i], want[1], "wsum of frame %d" % s)
    same_bits(big, stack, "the input is untouched")
    wide = torch.full((2, H, W + 11), 1.0, device="cuda")
    wide[:, :, 4:4 + W] = big[:2]
    crop = wide[:, :, 4:4 + W]
    got = ops.bilateral_depth(crop, **br.DEFAULTS)
    for s in range(2):
        same_bits(got[s], ref(H, W, 3, seed=s)[0], "cropped frame %d" % s)


def test_channels_first_and_batch_shapes(ops):
    """(B, L, 1, H, W) channels-first stack through its (B, L, H, W) view, and a (B, L, H, W) stack whose leading
    dimensions do not collapse to one stride (copied at the boundary): same bits"""
    H, W = 9, 65
    stack = np.stack([br.case(H, W, seed=s) for s in range(6)]).reshape(2, 3, 1, H, W)
    cf = dev(stack)
    got = ops.bilateral_depth(cf[:, :, 0], **br.DEFAULTS)
    assert got.shape == (2, 3, H, W)
    for s in range(6):
        same_bits(got[s // 3, s % 3], ref(H, W, 3, seed=s)[0], "frame %d" % s)
    odd = cf[:, ::2, 0]                      # (2, 2, H, W): strides (3 HW, 2 HW): not one stride
    got = ops.bilateral_depth(odd, **br.DEFAULTS)
    for b in range(2):
        for i, l in enumerate((0, 2)):
            same_bits(got[b, i], ref(H, W, 3, seed=3 * b + l)[0], "frame (%d, %d)" % (b, l))


def test_out_must_not_be_the_input(ops):
    from gradslam_amd import _C
    d = dev(br.case(9, 65))
    with pytest.raises(_C.HipExtensionError, match="alias"):
        ops.bilateral_depth(d, out=d)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ backward
def run_backward(ops, d, ob, radius):
    x = dev(d).requires_grad_(True)
    out = ops.bilateral_depth(x, **dict(br.DEFAULTS, radius=radius))
    out.backward(dev(ob))
    return host(x.grad), host(out)


@pytest.mark.parametrize("H,W,radius", br.BACKWARD_CASES)
def test_backward_within_the_bound_of_the_case(ops, H, W, radius):
    d, ob = br.case(H, W), br.weights(H, W)
    got, out = run_backward(ops, d, ob, radius)
    same_bits(out, ref(H, W, radius)[0], "the taped forward")
    want = br.adjoint(d, ob, **dict(br.DEFAULTS, radius=radius))
    gap = br.BACKWARD_GAP[br.backward_key(H, W, radius)]
    err = bc.rel_err(got, want)
    print("%s: rel err %.2e, gap %.2e, bound %.2e" % (br.backward_key(H, W, radius), err, gap, bc.kernel_bound(gap)))
    with np.errstate(invalid="ignore"):
        valid = d > 0
    assert np.array_equal(got[~valid], ob[~valid])            # the forward is the identity there
    assert (got[want == 0] == 0).all()
    assert err <= bc.kernel_bound(gap)
    again, _ = run_backward(ops, d, ob, radius)
    assert np.array_equal(br.bits(again), br.bits(got)), "two runs differ"


@pytest.mark.parametrize("H,W,radius", [(20, 70, 3), (67, 131, 8)])
def test_backward_of_a_sub_rectangle_touching_a_border(ops, H, W, radius):
    """out_bar lives on a rectangle in the top left corner: exactly zero where the reference is zero (further than the
    radius from the rectangle), within the bound elsewhere"""
    d = br.case(H, W)
    ob = np.zeros((H, W), np.float32)
    ob[:6, :9] = br.weights(H, W)[:6, :9]
    got, _ = run_backward(ops, d, ob, radius)
    kw = dict(br.DEFAULTS, radius=radius)
    want = br.adjoint(d, ob, **kw)
    assert (want[6 + radius:] == 0).all() and (want[:, 9 + radius:] == 0).all() and np.abs(want).max() > 0
    assert (got[want == 0] == 0).all()
    gap = bc.rel_err(br.adjoint(d, ob, dtype=np.float32, **kw), want)     # (the yardstick of THIS input, from NumPy alone)
    err = bc.rel_err(got, want)
    print("%dx%d r%d sub-rectangle: rel err %.2e, gap %.2e" % (H, W, radius, err, gap))
    assert err <= bc.kernel_bound(gap)


def test_backward_of_a_strided_stack(ops):
    H, W = 9, 65
    stack = np.stack([br.case(H, W, seed=s) for s in range(5)])
    big = dev(stack).requires_grad_(True)
    ob = np.stack([br.weights(H, W, seed=20 + i) for i in range(3)])
    ops.bilateral_depth(big[0:5:2], **br.DEFAULTS).backward(dev(ob))
    g = host(big.grad)
    assert (g[1] == 0).all() and (g[3] == 0).all()
    for i, s in enumerate((0, 2, 4)):
        want = br.adjoint(stack[s], ob[i], **br.DEFAULTS)
        assert bc.rel_err(g[s], want) <= bc.kernel_bound(br.BACKWARD_GAP[br.backward_key(H, W, 3)])


# ------------------------------------------------------------------------------------------ RGBDImages
def small_frames(gs, channels_first=False, requires_grad=False, L=2, nan_to=None):
    H, W = 9, 65
    depth = np.stack([br.case(H, W, seed=s) for s in range(L)])[None, ..., None]          # (1, L, H, W, 1)
    if nan_to is not None:
        depth = np.nan_to_num(depth, nan=nan_to)
    rgb = np.random.default_rng(5).random((1, L, H, W, 3), dtype=np.float32)
    K = T(br.plane_scene(H, W)[2]).view(1, 1, 4, 4).cuda()
    poses = torch.eye(4).view(1, 1, 4, 4).repeat(1, L, 1, 1).cuda()
    d, c = dev(depth), dev(rgb)
    if channels_first:
        d, c = d.permute(0, 1, 4, 2, 3).contiguous(), c.permute(0, 1, 4, 2, 3).contiguous()
    d.requires_grad_(requires_grad)
    return gs.RGBDImages(c, d, K, poses, channels_first=channels_first), depth


@pytest.mark.parametrize("channels_first", [False, True])
def test_rgbdimages_bilateral_filter(gs, channels_first):
    fr, depth = small_frames(gs, channels_first)
    _ = fr.vertex_map, fr.global_vertex_map, fr.valid_depth_mask            # caches that must not travel
    out = fr.bilateral_filter(**br.DEFAULTS)
    assert type(out) is type(fr) and out is not fr and out.channels_first == channels_first
    assert out.rgb_image is fr.rgb_image and out.intrinsics is fr.intrinsics and out.poses is fr.poses
    assert out.depth_image.shape == fr.depth_image.shape and out.shape == fr.shape
    assert out._vertex_map is None and out._normal_map is None and out._global_vertex_map is None and \
        out._global_normal_map is None and out._alpha_cache is None and out._valid_depth_mask is None
    assert fr._vertex_map is not None                                        # (the source keeps its own)
    got = out.depth_image[:, :, 0] if channels_first else out.depth_image[..., 0]
    for s in range(2):
        same_bits(got[0, s], ref(9, 65, 3, seed=s)[0], "frame %d" % s)
    same_bits(fr.depth_image.reshape(-1), depth.reshape(-1), "the source depth is untouched")
    # the maps of the result are those of a container built from the filtered depth
    fresh = gs.RGBDImages(fr.rgb_image, out.depth_image.clone(), fr.intrinsics, fr.poses, channels_first=channels_first)
    same_bits(out.vertex_map, host(fresh.vertex_map), "vertex map")        # (bits: the NaN pixel's vertex is NaN)
    same_bits(out.normal_map, host(fresh.normal_map), "normal map")
    assert torch.equal(out.valid_depth_mask, fr.valid_depth_mask)
    assert not np.array_equal(br.bits(host(out.vertex_map)), br.bits(host(fr.vertex_map)))


def test_gradient_reaches_the_depth_through_the_vertex_map(gs, ops):
    """loss = sum(w * z of the vertex map of the filtered frame): z = filtered depth at valid pixels, so the gradient at
    the raw depth is the filter's adjoint of w (masked).  The NaN pixel of the case is a hole here: the frame-map
    kernels are not under test, and a NaN vertex would make the loss NaN."""
    fr, depth = small_frames(gs, requires_grad=True, L=1, nan_to=0.0)
    d = depth[0, 0, ..., 0]
    out = fr.bilateral_filter(**br.DEFAULTS)
    assert out.depth_image.requires_grad
    vm = out.vertex_map                                  # (1, 1, H, W, 3)
    wz = br.weights(9, 65, seed=31)
    (vm[0, 0, ..., 2] * dev(wz)).sum().backward()
    g = host(fr.depth_image.grad)[0, 0, ..., 0]
    valid = d > 0
    ob = np.where(valid, wz, np.float32(0))              # vertex z = depth * valid
    want = np.where(valid, br.adjoint(d, ob, **br.DEFAULTS), 0.0)
    gap = bc.rel_err(np.where(valid, br.adjoint(d, ob, dtype=np.float32, **br.DEFAULTS), 0.0), want)
    err = bc.rel_err(g, want)
    print("through vertex_map: rel err %.2e, gap %.2e" % (err, gap))
    assert np.abs(g).max() > 0 and (g[~valid] == 0).all()
    assert err <= bc.kernel_bound(gap)


# ------------------------------------------------------------------------------------------ drivers
L_SEQ, H_SEQ, W_SEQ = 4, 48, 64
FILTER = dict(radius=2, sigma_space=1.5, sigma_range=0.05)


def noisy_sequence():
    s = make_sequence(L_SEQ, H_SEQ, W_SEQ, seed=3)
    d = s["depths"].copy()
    rng = np.random.default_rng(17)
    d = np.where(d > 0, d + np.float32(0.004) * rng.standard_normal(d.shape).astype(np.float32), d).astype(np.float32)
    return s, d


def frames_of(gs, s, depths):
    poses = T(s["poses"][None]).cuda()
    poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(depths[None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)


def step_loop(gs, slam, frames, expect_fast=True):
    pc, prev, rec, lives = gs.Pointclouds(device="cuda"), None, [], []
    for i in range(L_SEQ):
        live = frames[:, i]
        pc, p = slam.step(pc, live, prev, inplace=True)
        assert live.poses is not None and torch.equal(live.poses, p), "the caller's frame carries the recovered pose"
        prev = live
        lives.append(live)
        rec.append(host(p[0, 0]))
    if expect_fast:
        assert getattr(slam, "_step_plan", None) is not None, "the in-place loop must have taken the fast path"
    return pc, np.stack(rec), lives


def map_of(pc):
    """the four attributes of sequence 0 (an attribute the driver does not keep: an empty array)"""
    return [np.zeros(0, np.float32) if x is None else host(x[0])
            for x in (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)]


def same_run(a_map, a_poses, b_map, b_poses, what):
    for name, a, b in zip(("points", "normals", "colors", "ccounts"), a_map, b_map):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert np.array_equal(br.bits(a), br.bits(b)), "%s %s: %d of %d differ" % (what, name, (a != b).sum(), a.size)
    assert np.array_equal(br.bits(a_poses), br.bits(b_poses)), what + " poses"


@pytest.fixture(scope="module")
def runs(gs):
    """the noisy 4-frame sequence: PointFusion() on the pre-filtered frames (the reference of the driver tests),
    PointFusion(depth_filter=...) on the raw frames, and PointFusion() on the raw frames"""
    s, d = noisy_sequence()
    raw = frames_of(gs, s, d)
    pre = raw.bilateral_filter(**FILTER)
    want_pc, want_poses, _ = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda"), pre)
    got_pc, got_poses, lives = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda", depth_filter=FILTER), raw)
    plain_pc, plain_poses, _ = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda"), raw)
    return dict(s=s, d=d, raw=raw, pre=pre, want=(map_of(want_pc), want_poses), got=(map_of(got_pc), got_poses),
                plain=(map_of(plain_pc), plain_poses), lives=lives)


def test_filtering_pointfusion_equals_pointfusion_on_prefiltered_frames(runs):
    same_run(*runs["got"], *runs["want"], "fast path")
    # the filter changes the result (the comparison above is not vacuous) and leaves the caller's depth alone
    assert runs["got"][0][0].shape != runs["plain"][0][0].shape or \
        not np.array_equal(runs["got"][0][0], runs["plain"][0][0])
    same_bits(runs["raw"].depth_image.reshape(-1), runs["d"].reshape(-1), "the caller's depth")
    for live in runs["lives"]:
        assert live._vertex_map is None          # the maps were computed on the filtered copy, not on the caller's frame


def test_depth_filter_none_gives_todays_bits(gs, runs):
    pc, poses, _ = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda", depth_filter=None), runs["raw"])
    same_run(map_of(pc), poses, *runs["plain"], "depth_filter=None")


def test_forward_filters_the_same(gs, runs):
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", depth_filter=FILTER)
    pc, poses = slam(frames_of(gs, runs["s"], runs["d"]))
    same_run(map_of(pc), host(poses[0]), *runs["want"], "forward")


def test_icpslam_filters_the_same(gs, runs):
    a = step_loop(gs, gs.slam.ICPSLAM(odom="gradicp", device="cuda", depth_filter=FILTER), runs["raw"], expect_fast=False)
    b = step_loop(gs, gs.slam.ICPSLAM(odom="gradicp", device="cuda"), runs["pre"], expect_fast=False)
    same_run(map_of(a[0]), a[1], map_of(b[0]), b[1], "ICPSLAM")


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from tests.test_hip_bilateral import FILTER, frames_of, map_of, noisy_sequence, step_loop
s, d = noisy_sequence()
slam = gs.slam.PointFusion(odom="gradicp", device="cuda", depth_filter=FILTER)
pc, poses, _ = step_loop(gs, slam, frames_of(gs, s, d), expect_fast=False)
assert getattr(slam, "_step_plan", None) is None, "GRADSLAM_HIP_FASTPATH=0 must keep the fast path out"
m = map_of(pc)
np.savez(sys.argv[1], poses=poses, pts=m[0], nrm=m[1], col=m[2], cc=m[3])
"""


def test_generic_path_filters_the_same(runs, tmp_path):
    out = str(tmp_path / "generic.npz")
    subprocess.run([sys.executable, "-c", _CHILD % REPO, out], check=True, timeout=600,
                   env=dict(os.environ, GRADSLAM_HIP_FASTPATH="0"))
    z = np.load(out)
    same_run([z["pts"], z["nrm"], z["col"], z["cc"]], z["poses"], *runs["want"], "generic path")
