"""GPU tests of the model view (gs_render.hip -> gs_render_map_dc_f32 -> ops.render_map -> Pointclouds.render ->
metrics.depth_residual) against its NumPy restatement (tests/render_ref.py: the oracle's projection and point transform,
keys reduced with np.minimum.at).

The HIP maps are bit-identical to the oracle's and the render is a minimum over a set (independent of thread order), so
every comparison is for EQUAL BITS (+0 and -0 compare equal, as everywhere in the suite); the only tolerance is on the
float64 sums of the metric (n * 2^-53 relative for n <= H * W terms: rel = 1e-9)."""
import math

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from oracle import slam as oslam
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

T = torch.from_numpy
FIELDS = ("depth", "color", "normal", "confidence", "index")


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


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


@pytest.fixture(scope="module")
def small():
    """the 96x128 map: 6 frames, ground-truth odometry, oracle frame loop (20 410 surfels)"""
    s = make_sequence(6, 96, 128, seed=0)
    m, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gt")
    assert len(m) == 20410
    return s, m


@pytest.fixture(scope="module")
def big():
    """a 480x640 map of two frames"""
    s = make_sequence(2, 480, 640, seed=5)
    m, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gt")
    return s, m


def same_views(got, want, what=""):
    """got: RenderedViews of one view (tensors); want: render_ref.Rendered"""
    for k in FIELDS:
        a, b = host(getattr(got, k)), getattr(want, k)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), "%s %s: %d of %d differ" % (what, k, (a != b).sum(), a.size)
    # depth also bit for bit (it is never -0)
    assert np.array_equal(host(got.depth).view(np.uint32), want.depth.view(np.uint32)), what


def hip_render(ops, m, poses, K, H, W, **kw):
    return ops.render_map(dev(m.points), dev(m.normals), dev(m.colors), dev(m.ccounts), dev(poses), dev(K), H, W, **kw)


def view(r, v):
    return type(r)(*[t[v] for t in r])


def off_pose(pose):
    """a pose that is not one of the sequence: 4 degrees of yaw and a translation on top of `pose`"""
    a = math.radians(4.0)
    D = np.eye(4, dtype=np.float64)
    D[0, 0], D[0, 2], D[2, 0], D[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    D[:3, 3] = (0.03, -0.02, 0.05)
    return (pose.astype(np.float64) @ D).astype(np.float32)


def scaled_K(K, f):
    K = K.copy()
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K[0, 0] * f, K[1, 1] * f, K[0, 2] * f, K[1, 2] * f
    return K


def mirrored_K(K, H):
    """negative fy with cy mirrored: v' = (H - 1) - v, the view stays in the window upside down"""
    K = K.copy()
    K[1, 1], K[1, 2] = -K[1, 1], (H - 1) - K[1, 2]
    return K


CASES = {
    # name: (map, geometry, filters)
    "seq_pose": ("small", "pose3", {}),
    "off_pose": ("small", "off", {}),
    "two_frames_640": ("big", "pose1", {}),
    "two_frames_640_off_r1": ("big", "off", {"radius": 1}),
    "resized_1p5": ("small", "resized", {}),
    "resized_1p5_r2": ("small", "resized", {"radius": 2}),
    "negative_fy": ("small", "neg_fy", {}),
    "radius1": ("small", "pose3", {"radius": 1}),
    "radius2": ("small", "off", {"radius": 2}),
    "min_confidence": ("small", "pose3", {"min_confidence": "median"}),
    "cull_backfaces": ("small", "off", {"cull_backfaces": True}),
    "all_filters": ("small", "off", {"radius": 1, "min_confidence": "median", "cull_backfaces": True}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_equals_restatement(ops, small, big, case):
    which, geom, kw = CASES[case]
    s, m = small if which == "small" else big
    H, W = s["depths"].shape[1:3]
    K = s["intrinsics"][0]
    last = len(s["poses"]) - 1
    pose = {"pose3": s["poses"][min(3, last)], "pose1": s["poses"][1], "off": off_pose(s["poses"][1]),
            "resized": s["poses"][min(2, last)], "neg_fy": s["poses"][min(4, last)]}[geom]
    if geom == "resized":
        H, W, K = (H * 3) // 2, (W * 3) // 2, scaled_K(K, 1.5)
    if geom == "neg_fy":
        K = mirrored_K(K, H)
    kw = dict(kw)
    if kw.get("min_confidence") == "median":
        cc = np.sort(m.ccounts.reshape(-1))
        kw["min_confidence"] = float(cc[len(cc) // 2])
        assert cc[0] < kw["min_confidence"] < cc[-1]
    want = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, **kw)
    got = hip_render(ops, m, pose, K, H, W, **kw)
    assert (want.index >= 0).mean() > 0.1, "the view must show the scene"
    if kw.get("cull_backfaces") or kw.get("min_confidence"):
        plain = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, radius=kw.get("radius", 0))
        assert not np.array_equal(plain.index, want.index), "the filter must change something"
    if geom == "neg_fy":
        up = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, s["intrinsics"][0], H, W)
        assert abs(int((up.index >= 0).sum()) - int((want.index >= 0).sum())) < 0.02 * H * W
    same_views(view(got, 0), want, case)


def test_duplicated_rows_lowest_index_wins(ops, small):
    s, m = small
    H, W, K, pose = 96, 128, s["intrinsics"][0], s["poses"][2]
    n = len(m)
    dup = np.arange(0, n, 7)

    class M:
        pass
    for order in ("copies_last", "copies_first"):
        q = M()
        for k in ("points", "normals", "colors", "ccounts"):
            a = getattr(m, k)
            setattr(q, k, np.concatenate([a, a[dup]] if order == "copies_last" else [a[dup], a]))
        # the copies carry other colours: a wrong winner shows in the colour image as well
        if order == "copies_last":
            q.colors[n:] += 1.0
        else:
            q.colors[:len(dup)] += 1.0
        want = rr.render(q.points, q.normals, q.colors, q.ccounts, pose, K, H, W)
        got = view(hip_render(ops, q, pose, K, H, W), 0)
        same_views(got, want, order)
        idx = host(got.index)
        if order == "copies_last":
            assert idx.max() < n, "a copy at a higher index won a pixel"
            base = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W)
            assert np.array_equal(idx, base.index)
        else:
            won_by_original = (idx >= len(dup)) & ((idx - len(dup)) % 7 == 0)
            assert not won_by_original.any(), "an original at a higher index beat its copy"
            assert (idx[idx >= 0] < len(dup)).sum() > 100


def test_rows_behind_the_camera_or_outside_the_window_leave_the_pixel_empty(ops):
    H, W = 24, 32
    K = np.array([[30, 0, 16, 0], [0, 30, 12, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    pose = np.eye(4, dtype=np.float32)
    pts = np.array([[0, 0, -1], [0.1, 0.1, -2], [0, 0, 0],          # behind / at the camera
                    [5, 0, 1], [-5, 0, 1], [0, 5, 1], [0, -5, 1],   # outside the window
                    [np.nan, 0, 1], [0, 0, np.nan]], np.float32)
    nrm = np.tile(np.array([[0, 0, -1]], np.float32), (len(pts), 1))
    col = np.full((len(pts), 3), 9, np.float32)
    cc = np.ones((len(pts), 1), np.float32)
    got = view(ops.render_map(dev(pts), dev(nrm), dev(col), dev(cc), dev(pose), dev(K), H, W, radius=2), 0)
    assert not host(got.depth).any() and not host(got.color).any() and not host(got.normal).any()
    assert not host(got.confidence).any() and (host(got.index) == -1).all()
    same_views(got, rr.render(pts, nrm, col, cc, pose, K, H, W, radius=2))
    # one row in front: exactly its square is filled
    pts[0] = (0, 0, 2)
    got = view(ops.render_map(dev(pts), dev(nrm), dev(col), dev(cc), dev(pose), dev(K), H, W, radius=1), 0)
    idx = host(got.index)
    assert (idx == 0).sum() == 9 and (idx[11:14, 15:18] == 0).all() and ((idx == 0) | (idx == -1)).all()
    assert (host(got.depth)[11:14, 15:18] == 2.0).all()
    same_views(got, rr.render(pts, nrm, col, cc, pose, K, H, W, radius=1))


def test_empty_map(ops):
    H, W = 8, 12
    e3, e1 = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 1), device="cuda")
    K = torch.eye(4, device="cuda")
    got = ops.render_map(e3, e3, e3, e1, torch.eye(4, device="cuda").repeat(2, 1, 1), K, H, W)
    assert got.depth.shape == (2, H, W, 1) and got.index.shape == (2, H, W) and got.index.dtype == torch.int64
    assert not host(got.depth).any() and not host(got.color).any() and (host(got.index) == -1).all()
    # a buffer with rows but a device count of zero
    p = torch.tensor([[0.0, 0.0, 1.0]] * 4, device="cuda")
    got = ops.render_map(p, p, p, p[:, :1].contiguous(), torch.eye(4, device="cuda"), K, H, W,
                         n_dev=torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert (host(got.index) == -1).all() and not host(got.depth).any()


def test_rows_beyond_the_device_count_do_not_appear(ops, small):
    s, m = small
    H, W, K, pose = 96, 128, s["intrinsics"][0], s["poses"][1]
    n, cap = len(m), len(m) + 5000
    Tinv, _ = rr.camera_inverse(pose)
    # filler rows: a plane 0.3 m in front of the camera (nearer than the scene: it would win every pixel it covers)
    rng = np.random.default_rng(3)
    cam = np.stack([rng.uniform(-0.1, 0.1, cap - n), rng.uniform(-0.1, 0.1, cap - n), np.full(cap - n, 0.3)], -1)
    filler = (cam @ pose[:3, :3].T.astype(np.float64) + pose[:3, 3]).astype(np.float32)
    bufs = []
    for a, fill in ((m.points, filler), (m.normals, np.tile(np.float32([[0, 0, -1]]), (cap - n, 1))),
                    (m.colors, np.full((cap - n, 3), 255, np.float32)), (m.ccounts, np.full((cap - n, 1), 50, np.float32))):
        bufs.append(dev(np.concatenate([a, fill])))
    want = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, radius=1)
    n_dev = torch.tensor([n], dtype=torch.int64, device="cuda")
    with_count = view(ops.render_map(*bufs, dev(pose), dev(K), H, W, n_dev=n_dev, radius=1), 0)
    same_views(with_count, want, "n_dev given")
    sliced = view(ops.render_map(*[b[:n] for b in bufs], dev(pose), dev(K), H, W, radius=1), 0)
    same_views(sliced, want, "n_dev not given")
    # a device count above the buffer is clamped to the buffer; and the filler does show when it is counted in
    whole = view(ops.render_map(*bufs, dev(pose), dev(K), H, W, radius=1,
                                n_dev=torch.tensor([cap + 100], dtype=torch.int64, device="cuda")), 0)
    same_views(whole, rr.render(*[host(b) for b in bufs], pose, K, H, W, radius=1), "count above the bound")
    assert (host(whole.index) >= n).sum() > 100


def test_batch_and_views_equal_single_calls(ops, small, big):
    s, m = small
    H, W = 96, 128
    K0 = s["intrinsics"][0]
    K1 = scaled_K(K0, 0.9)
    n1 = 9001
    poses = np.stack([np.stack([s["poses"][0], s["poses"][3], off_pose(s["poses"][5])]),
                      np.stack([off_pose(s["poses"][0]), s["poses"][2], s["poses"][4]])])
    full = [dev(getattr(m, k)) for k in ("points", "normals", "colors", "ccounts")]
    n_dev = torch.tensor([n1], dtype=torch.int64, device="cuda")
    maps = [tuple(full) + (None, None), tuple(full) + (len(m), n_dev)]   # ragged: 20 410 rows and the first 9 001 of them
    kw = dict(radius=1, cull_backfaces=True)
    got = ops.render_map_batch(maps, dev(poses), dev(np.stack([K0, K1])), H, W, **kw)
    again = ops.render_map_batch(maps, dev(poses), dev(np.stack([K0, K1])), H, W, **kw)
    for k in FIELDS:
        assert getattr(got, k).shape[:4] == (2, 3, H, W)
        assert torch.equal(getattr(got, k), getattr(again, k)), "two runs of the same call differ: " + k
    for b, (Kb, nb) in enumerate(((K0, len(m)), (K1, n1))):
        single = ops.render_map(*[t[:nb] for t in full], dev(poses[b]), dev(Kb), H, W, **kw)
        for k in FIELDS:
            assert torch.equal(getattr(got, k)[b], getattr(single, k)), (b, k)
        for v in range(3):
            one = ops.render_map(*[t[:nb] for t in full], dev(poses[b, v]), dev(Kb), H, W, **kw)
            for k in FIELDS:
                assert torch.equal(getattr(single, k)[v], getattr(one, k)[0]), (b, v, k)
            same_views(view(one, 0), rr.render(m.points[:nb], m.normals[:nb], m.colors[:nb], m.ccounts[:nb], poses[b, v], Kb,
                                               H, W, **kw), "b%d v%d" % (b, v))


def test_more_views_than_one_launch_serves(ops, small):
    s, m = small
    H, W, K = 96, 128, s["intrinsics"][0]
    poses = np.stack([s["poses"][i] for i in range(6)] + [off_pose(s["poses"][i]) for i in (0, 2, 5)])   # 9 > 2 x 4
    got = hip_render(ops, m, poses, K, H, W)
    assert got.depth.shape == (9, H, W, 1)
    for v in range(len(poses)):
        one = hip_render(ops, m, poses[v], K, H, W)
        for k in FIELDS:
            assert torch.equal(getattr(got, k)[v], getattr(one, k)[0]), (v, k)
    same_views(view(got, 7), rr.render(m.points, m.normals, m.colors, m.ccounts, poses[7], K, H, W), "view 7")


def test_out_buffers_and_detached_warning(ops, small):
    s, m = small
    H, W, K, pose = 96, 128, s["intrinsics"][0], s["poses"][1]
    ref = hip_render(ops, m, pose, K, H, W)
    out = tuple(torch.full_like(t, 7) for t in ref)
    ret = hip_render(ops, m, pose, K, H, W, out=out)
    for a, b, c in zip(ret, out, ref):
        assert a.data_ptr() == b.data_ptr() and torch.equal(a, c)
    p = dev(m.points).requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        r = ops.render_map(p, dev(m.normals), dev(m.colors), dev(m.ccounts), dev(pose), dev(K), H, W)
    assert not r.depth.requires_grad and torch.equal(r.depth, ref.depth)


def _frames(gs, s):
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(),
                         T(s["poses"][None]).cuda())


def test_pointclouds_render_equals_restatement_on_the_oracle_map(gs, small):
    s, m = small
    H, W = 96, 128
    frames = _frames(gs, s)
    pc, _ = gs.slam.PointFusion(odom="gt", device="cuda")(frames)
    poses = np.stack([s["poses"][0], s["poses"][4], off_pose(s["poses"][2])])
    rendered, extras = pc.render(frames.intrinsics, dev(poses[None]), H, W, return_extras=True)
    assert isinstance(rendered, gs.RGBDImages) and rendered.shape == (1, 3, H, W)
    assert torch.equal(rendered.poses, dev(poses[None])) and torch.equal(rendered.intrinsics, frames.intrinsics)
    assert set(extras) == {"normal", "confidence", "index"}
    for v in range(3):
        want = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[v], s["intrinsics"][0], H, W)
        got = type(want)(rendered.depth_image[0, v], rendered.rgb_image[0, v], extras["normal"][0, v],
                         extras["confidence"][0, v], extras["index"][0, v], None)
        same_views(got, want, "view %d" % v)
    only = pc.render(frames.intrinsics, dev(poses[None]), H, W, radius=1)
    assert isinstance(only, gs.RGBDImages)
    want = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[1], s["intrinsics"][0], H, W, radius=1)
    assert np.array_equal(host(only.depth_image[0, 1]), want.depth) and np.array_equal(host(only.rgb_image[0, 1]), want.color)


def test_render_between_steps_leaves_the_frame_loop_alone(gs):
    """PointFusion.step with a render between the steps: same poses and map bits as without, the map tensors keep their
    addresses across every render, device-side counts stay on the device (the fast path's preconditions)."""
    L, H, W = 6, 96, 128
    s = make_sequence(L, H, W, seed=7)

    def run(with_render):
        poses = T(s["poses"][None]).cuda()
        poses[:, 1:] = poses[:, :1]   # (only the first pose is given: the others are recovered)
        frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
        slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
        pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
        for i in range(L):
            live = frames[:, i]
            pc, p = slam.step(pc, live, prev, inplace=True)
            prev = live
            rec.append(host(p[:, 0]))
            if with_render:
                ptrs = [t[0].data_ptr() for t in pc._buf.values()]
                dcount = dict(pc._dcount)
                r = pc.render(frames.intrinsics, p, H // 2, W // 2, radius=1)
                assert bool((r.depth_image > 0).any())
                assert ptrs == [t[0].data_ptr() for t in pc._buf.values()], "render moved a map buffer"
                assert pc._dcount == dcount, "render resolved a device-side count"
                if i >= 2:
                    assert pc._dcount, "the counts of an in-place map live on the device"
        return rec + [np.concatenate([host(x) for x in getattr(pc, k)]) for k in
                      ("points_list", "normals_list", "colors_list", "features_list")]

    a, b = run(False), run(True)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))


def test_depth_residual_equals_numpy(gs, small):
    from gradslam_amd.metrics import depth_residual
    s, m = small
    frames = _frames(gs, s)
    pc, _ = gs.slam.PointFusion(odom="gt", device="cuda")(frames)
    for kw in ({}, {"radius": 1, "cull_backfaces": True}):
        got = depth_residual(pc, frames, **kw)
        for k in ("coverage", "mean_abs", "median_abs", "rmse", "pixels"):
            assert tuple(got[k].shape) == (1, 6) and got[k].dtype == torch.float64 and got[k].device.type == "cpu"
        for f in range(6):
            r = rr.render(m.points, m.normals, m.colors, m.ccounts, s["poses"][f], s["intrinsics"][0], 96, 128, **kw)
            want = rr.residual_stats(r.depth, s["depths"][f])
            print("frame %d %s: coverage %.6f mean_abs %.6g median_abs %.6g rmse %.6g" % (
                f, kw, want["coverage"], want["mean_abs"], want["median_abs"], want["rmse"]))
            assert float(got["coverage"][0, f]) == want["coverage"] and float(got["pixels"][0, f]) == want["pixels"]
            for k in ("mean_abs", "median_abs", "rmse"):
                assert float(got[k][0, f]) == pytest.approx(want[k], rel=1e-9), (f, k)
        if not kw:
            assert float(got["coverage"].min()) > 0.98 and float(got["median_abs"].max()) < 2e-3
