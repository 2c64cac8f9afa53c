"""GPU tests of the projective ICP's outlier mask (gs_picp_outliers.hip -> gs_picp_outlier_classes_batch_f32 /
gs_region_mask_u8 -> ops.region_mask / ops.projective_icp_outliers* -> ProjectiveICPOdometryProvider(outlier_mask=...) ->
PointFusion(odom_outlier_mask=..., fuse_outliers=False)), held bit for bit to the NumPy restatement
(tests/outlier_mask_ref.py) at the smallest shapes that can go wrong:

    region pass   1 x 1; 5 x 7 (below a 32 x 32 tile); 37 x 53 and 65 x 33 (odd sizes that straddle tile borders, with a
                  corridor that grows across one); B = 3 and B = 9; grow 0, 1, 3, 16 (the halo from 1 to 17 cells);
                  min_support 1, 6, 9
    class pass    the 60 x 80 wave scene with the moved block at the first solve's pose: 4 800 pixels, 18 chunks and a
                  tail of 192; a device count below the rows the index image names; special weights; a floor above every
                  residual; an empty map view; B = 9 past one launch group of 8"""
import math

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import outlier_mask_ref as om
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr
from tests import picp_weighted_ref as wr
from tests.test_hip_picp import FUSION, bits, dev, frames_of, host, map_rows, three_sequences
from tests.test_outlier_mask_cpu import E, S, corridor, random_classes, random_depth

pytestmark = pytest.mark.gpu
F = np.float32
K_HUBER = sr.K_HUBER


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


def same(got, want):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    if got.dtype.itemsize == 1:
        return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ 1. the region pass
def region_images(h, w, n, grow):
    """n class images (h, w) with their depths: random ones and, where the image has the room, a corridor of grow + 2
    eligible pixels from one seed that crosses the tile border at 32, along a row (image 1) and along a column (image 2)"""
    cls = np.stack([random_classes((h, w), 10 + i) for i in range(n)])
    d = np.stack([random_depth((h, w), 40 + i) for i in range(n)])
    ends = {}
    if w >= 25 + grow + 3 and h > 20:
        cls[1], d[1] = 0, 1
        cls[1, 20, 25], cls[1, 20, 26:25 + grow + 3] = S, E
        ends[1] = (20, slice(25, 25 + grow + 1)), (20, slice(25 + grow + 1, 25 + grow + 3))
    if h >= 25 + grow + 3 and w > 10:
        cls[2], d[2] = 0, 1
        cls[2, 25, 10], cls[2, 26:25 + grow + 3, 10] = S, E
        ends[2] = (slice(25, 25 + grow + 1), 10), (slice(25 + grow + 1, 25 + grow + 3), 10)
    return cls, d, ends


@pytest.mark.parametrize("grow", [0, 1, 3, 16])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (37, 53), (65, 33)])
def test_region_mask_bit_for_bit(ops, h, w, grow):
    for n in (3, 9):
        cls, d, ends = region_images(h, w, n, grow)
        for k in (1, 6, 9):
            want = np.stack([om.region_mask(cls[i], d[i], k, grow) for i in range(n)])
            got = ops.region_mask(dev(cls), dev(d), min_support=k, grow=grow)
            assert got.dtype == torch.uint8 and same(got, want), (n, k, np.argwhere(host(got) != want)[:5])
            if k == 1:
                assert (h, w) == (1, 1) or want.any()
                for i, (reached, beyond) in ends.items():      # the corridor: up to step grow and no further
                    assert want[i][reached].all() and not want[i][beyond].any() and want[i].sum() == grow + 1
    if (h, w) in ((37, 53), (65, 33)) and grow == 16:
        assert ends, "a growth path crosses the tile border at 32"
    # any leading shape, and the same bits on a second run
    cls, d, _ = region_images(h, w, 6, grow)
    got = ops.region_mask(dev(cls).view(2, 3, h, w), dev(d).view(2, 3, h, w), min_support=2, grow=grow)
    again = ops.region_mask(dev(cls).view(2, 3, h, w), dev(d).view(2, 3, h, w), min_support=2, grow=grow)
    want = np.stack([om.region_mask(cls[i], d[i], 2, grow) for i in range(6)]).reshape(2, 3, h, w)
    assert same(got, want) and same(again, want)
    one = ops.region_mask(dev(cls[0]), dev(d[0]), min_support=2, grow=grow)
    assert same(one, want[0, 0])


def test_region_mask_depth_gap(ops):
    cls = np.zeros((3, 4), np.uint8)
    cls[1, 0], cls[1, 1:] = S, E
    d = np.ones((3, 4), F)
    d[1, 1] = F(1.25)
    d[1, 2] = d[1, 3] = np.nextafter(F(1.25), F(2))
    cases = [d.copy()]
    d[1, 1] = d[1, 2]
    cases.append(d.copy())
    d[1, 1] = np.nan
    cases.append(d.copy())
    for d in cases:
        want = om.region_mask(cls, d, 1, 3, 0.25)
        assert same(ops.region_mask(dev(cls), dev(d), min_support=1, grow=3, grow_depth=0.25), want)
    assert om.region_mask(cls, cases[0], 1, 3, 0.25)[1].tolist() == [1, 1, 1, 1]
    assert om.region_mask(cls, cases[1], 1, 3, 0.25)[1].tolist() == [1, 0, 0, 0]
    # the default grow_depth as the float32 the library takes
    cls, dd = corridor(3, 3, 12)
    dd[3, 4] = F(1) + F(0.02)
    for gd in (0.02, 0.0200001, 0.0199999):
        assert same(ops.region_mask(dev(cls), dev(dd), min_support=1, grow=3, grow_depth=gd), om.region_mask(cls, dd, 1, 3, gd))


# ------------------------------------------------------------------------------------------ 2. the class pass
_FX = {}


def moved():
    """the 60 x 80 wave scene with the moved block and the pose the first solve ends at (10 iterations, huber_k, stride 4)"""
    if not _FX:
        fx = rr.moved_block(pr.convergence_fixture())
        T1 = wr.solve(*pr.args_of(fx), None, fx["T0"], stride=4, numiters=10, huber_k=K_HUBER)[0]
        _FX["fx"] = dict(fx, T1=T1)
    return _FX["fx"]


def outliers_call(ops, fx, T, n_dev=None, **kw):
    t = [dev(fx[k]) for k in pr.ARGS[:-1]]
    return ops.projective_icp_outliers(*t, dev(T), n_dev=n_dev, return_classes=True, return_thresholds=True, **kw)


def check(got, want):
    mask, cls, th = got
    assert same(th, want.thresholds), (host(th), want.thresholds)
    assert same(cls, want.classes), np.argwhere(host(cls) != want.classes)[:5]
    assert same(mask, want.mask), np.argwhere(host(mask) != want.mask)[:5]


@pytest.mark.parametrize("rule", [dict(), dict(grow=8), dict(hi=2.0, lo=1.0, min_support=3, grow=2, grow_depth=0.05),
                                  dict(floor=0.0015)])
def test_outliers_bit_for_bit_at_the_first_solves_pose(ops, rule):
    fx = moved()
    want = om.outliers(*pr.args_of(fx), fx["T1"], **rule)
    if not rule:
        assert want.mask[rr.BLOCK].sum() > 500 and (want.classes == E).any()
    check(outliers_call(ops, fx, fx["T1"], **rule), want)
    mask = outliers_call(ops, fx, fx["T1"], **rule)[0]
    only = ops.projective_icp_outliers(*[dev(fx[k]) for k in pr.ARGS[:-1]], dev(fx["T1"]), **rule)
    assert same(mask, want.mask) and same(only, want.mask)


def test_outliers_with_stale_index_entries(ops):
    fx = moved()
    keep = fx["count"] - 400
    want = om.outliers(*pr.args_of(dict(fx, count=keep)), fx["T1"])
    assert (want.code == 3).sum() >= 300
    n_dev = torch.tensor([keep], dtype=torch.int64, device="cuda")
    check(outliers_call(ops, fx, fx["T1"], n_dev=n_dev), want)
    assert not np.array_equal(want.classes, om.outliers(*pr.args_of(fx), fx["T1"]).classes)


def test_outliers_with_special_weights(ops):
    fx = moved()
    w = wr.special_weights((60, 80))
    want = om.outliers(*pr.args_of(fx), fx["T1"], w, grow=3)
    assert (want.code == wr.MASKED).sum() > 500 and want.mask.any() and not want.mask[want.code == wr.MASKED].any()
    check(outliers_call(ops, fx, fx["T1"], pixel_weights=dev(w), grow=3), want)
    ones = outliers_call(ops, fx, fx["T1"], pixel_weights=torch.ones(60, 80).cuda(), grow=3)
    check(ones, om.outliers(*pr.args_of(fx), fx["T1"], grow=3))


def test_outliers_with_a_floor_above_every_residual_and_an_empty_view(ops):
    fx = moved()
    want = om.outliers(*pr.args_of(fx), fx["T1"], floor=1.0, min_support=1)
    assert want.thresholds.tolist() == [1.0, 1.0]
    assert np.array_equal(want.mask != 0, np.isin(want.code, (4, 5)))          # only the gates' outliers are left
    check(outliers_call(ops, fx, fx["T1"], floor=1.0, min_support=1), want)
    # an empty view: no row is valid, no pixel is used, both thresholds +0.0, the mask all zero
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    for floor in (0.0, 0.001):
        want = om.outliers(*pr.args_of(dict(fx, count=0)), fx["T1"], floor=floor, grow=4)
        assert not want.mask.any() and want.thresholds.tobytes() == np.zeros(2, F).tobytes()
        check(outliers_call(ops, fx, fx["T1"], n_dev=zero, floor=floor, grow=4), want)


def test_outliers_batch_of_nine_with_mixed_sequences(ops):
    seqs = three_sequences()
    nine = [seqs[i % 3] for i in range(9)]
    poses = [np.asarray(q["gt"] if i % 2 else q["T0"], F) for i, q in enumerate(nine)]
    wts = [None if i in (1, 7) else wr.random_weights((60, 80), seed=20 + i, patch=(slice(5 * i, 5 * i + 12), slice(10, 40)))
           for i in range(9)]
    st = lambda k: torch.stack([dev(q[k]) for q in nine])   # noqa: E731
    maps = [(dev(q["points"]), dev(q["normals"]), None, None, None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in nine]
    rule = dict(grow=2, min_support=4)
    mask, cls, th = ops.projective_icp_outliers_batch(
        st("vertex"), st("normal"), st("depth"), st("K"), st("index"), st("model_pose"), maps,
        torch.stack([dev(T) for T in poses]), pixel_weights=[None if w is None else dev(w) for w in wts],
        return_classes=True, return_thresholds=True, **rule)
    assert tuple(mask.shape) == (9, 60, 80) and tuple(th.shape) == (9, 2)
    for i, q in enumerate(nine):
        want = om.outliers(*pr.args_of(q), poses[i], wts[i], **rule)
        check((mask[i], cls[i], th[i]), want)
    assert len({host(mask[i]).tobytes() for i in range(9)}) >= 6 and host(mask).any()
    # without any weights: the unweighted kernels
    mask0 = ops.projective_icp_outliers_batch(st("vertex")[:3], st("normal")[:3], st("depth")[:3], st("K")[:3],
                                              st("index")[:3], st("model_pose")[:3], maps[:3],
                                              torch.stack([dev(T) for T in poses[:3]]), **rule)
    for i in range(3):
        assert same(mask0[i], om.outliers(*pr.args_of(nine[i]), poses[i], None, **rule).mask), i


# ------------------------------------------------------------------------------------------ 3. the provider
SEEDS, H, W = (0, 1), 60, 80
RULE = dict(hi=2.5, lo=1.25, min_support=4, grow=2, refine_iters=3)


@pytest.fixture(scope="module")
def sequences():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(4, H, W, seed=s) for s in SEEDS]


def moved_frames(gs, sequences, first_pose_only=False):
    """the sequences with a block of every frame from the second on 4 cm nearer: something for the mask to find"""
    seqs = []
    for q in sequences:
        q = dict(q)
        d = q["depths"].copy()
        blk = d[1:, 15:38, 20:51]
        d[1:, 15:38, 20:51] = np.where(blk > 0, blk - F(rr.SHIFT), blk)
        q["depths"] = d
        seqs.append(q)
    return frames_of(gs, seqs, first_pose_only=first_pose_only)


def two_frame_map(gs, frames):
    slam = gs.slam.PointFusion(odom="gt", device="cuda", **FUSION)
    pc = gs.Pointclouds(device="cuda")
    for s in range(2):
        pc, _ = slam.step(pc, frames[:, s], None, inplace=True)
    return pc


def band_weights(frames):
    z = frames.to_channels_last().depth_image[..., 0]
    w = torch.where(z > 0, 1.0 / (0.5 + z), torch.zeros_like(z))
    w = w.clone()
    w[..., :6] = 0
    return w


def composed(ops, pc, live, prev, rule, weights=None, differentiable=False, deterministic=None, color_weight=0.0,
             stride=1, numiters=10, **robust):
    """the hand composition of the ops: render, solve, mask at the solve's poses, the masked weights, refine_iters more
    iterations from those poses.  Returns (poses (B, 4, 4), mask (B, H, W) bool)"""
    B = live.shape[0]
    fr = live.to_channels_last()
    K = fr.intrinsics[:, 0].contiguous().float()
    p0 = prev.reshape(B, 4, 4).contiguous().float()
    maps = pc._map_rows(("points", "normals"))
    view_maps = [m._replace(normals=None, points=m.points.detach()) for m in maps]
    if color_weight > 0:
        view_maps = [m._replace(colors=pc._buf["colors"][b]) for b, m in enumerate(view_maps)]
    view = ops.render_map_batch(view_maps, p0.detach().view(B, 1, 4, 4), K, H, W)
    args = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, view.index[:, 0], p0.detach(), maps)
    rule = dict(rule)
    refine_iters = rule.pop("refine_iters")

    def solve(init, w, iters):
        if color_weight > 0:
            model = ops.model_intensity(view.color[:, 0], view.index[:, 0])
            return ops.projective_icp_color_batch(*args, init, fr.rgb_image[:, 0], model, color_weight=color_weight,
                                                  stride=stride, numiters=iters, pixel_weights=w, **robust)
        return ops.projective_icp_batch(*args, init, stride=stride, numiters=iters, pixel_weights=w,
                                        differentiable=differentiable, deterministic=deterministic, **robust)
    first = solve(p0, weights, numiters)
    with torch.no_grad():
        mask = ops.projective_icp_outliers_batch(*args, first, pixel_weights=weights, **rule).bool()
    base = torch.ones((B, H, W), device="cuda") if weights is None else weights
    masked = torch.where(mask, torch.zeros((), device="cuda"), base)
    return solve(first, masked, refine_iters), mask


SOLVES = {"plain": dict(), "huber_k": dict(huber_k=K_HUBER), "color": dict(color_weight=0.2, huber_k=K_HUBER),
          "weights": dict(huber_k=K_HUBER, huber_delta=0.001)}


@pytest.mark.parametrize("which", sorted(SOLVES))
def test_localize_equals_the_hand_composition(gs, ops, sequences, which):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    frames = moved_frames(gs, sequences)
    pc = two_frame_map(gs, frames)
    live, prev = frames[:, 2], frames.poses[:, 1:2].clone()
    f = band_weights if which == "weights" else None
    prov = ProjectiveICPOdometryProvider(numiters=6, stride=2, outlier_mask=RULE, pixel_weights=f, **SOLVES[which])
    got = prov.localize(pc, live, prev)
    w = None if f is None else f(live).reshape(len(SEEDS), H, W)
    want, mask = composed(ops, pc, live, prev, RULE, weights=w, stride=2, numiters=6, **SOLVES[which])
    assert tuple(got.shape) == (len(SEEDS), 1, 4, 4) and same(got[:, 0], host(want))
    assert prov.last_outlier_mask.dtype == torch.bool and same(prov.last_outlier_mask, host(mask))
    assert host(mask).any()
    if which != "color":     # (the sequences' colours are per-frame noise: the joint solve's pose, and so its mask, say nothing)
        assert host(mask)[:, 15:38, 20:51].mean() > 0.5 and host(mask).mean() < 0.3     # it found the block
    # without the keyword: the calls and the bits of today, and no mask
    plain = ProjectiveICPOdometryProvider(numiters=6, stride=2, pixel_weights=f, **SOLVES[which])
    assert not same(plain.localize(pc, live, prev), host(got)) and plain.last_outlier_mask is None
    # the mask is that of the restated rule on the device's own inputs at the first solve's pose
    if which == "huber_k":
        first = plain.localize(pc, live, prev)
        fr = live.to_channels_last()
        m0 = pc._map_rows(("points", "normals"))[0]
        view = ops.render_map_batch([m0._replace(normals=None)], prev[:1].reshape(1, 1, 4, 4), fr.intrinsics[:1, 0].contiguous(),
                                    H, W)
        n = int(m0.n_dev.item()) if m0.n_dev is not None else m0.n_bound
        rule = {k: v for k, v in RULE.items() if k != "refine_iters"}
        want0 = om.outliers(host(fr.vertex_map[0, 0]), host(fr.normal_map[0, 0]), host(fr.depth_image[0, 0, ..., 0]),
                            host(fr.intrinsics[0, 0]), host(view.index[0, 0]), host(prev[0, 0]), host(m0.points),
                            host(m0.normals), n, host(first[0, 0]), **rule)
        assert same(prov.last_outlier_mask[0].to(torch.uint8), want0.mask)


def test_localize_on_the_tape_equals_the_hand_composition(gs, ops, sequences):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    B = len(SEEDS)
    Tb = torch.stack([dev(bc.weights((4, 4), 60 + b)) for b in range(B)])
    grads = []
    for how in ("provider", "composed"):
        frames = moved_frames(gs, sequences)
        frames.depth_image.requires_grad_(True)                  # the map itself is on the tape
        pc = two_frame_map(gs, frames)
        live = frames[:, 2]
        prev = frames.poses[:, 1:2].clone().requires_grad_(True)
        vertex = live.to_channels_last().vertex_map
        scale = torch.full((B, H, W), 0.75, device="cuda").requires_grad_(True)
        f = lambda fr, s=scale: band_weights(fr).reshape(B, H, W) * s   # noqa: E731
        P, N = list(pc._buf["points"]), list(pc._buf["normals"])
        assert all(t.requires_grad for t in P)
        if how == "provider":
            prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, outlier_mask=RULE, pixel_weights=f, huber_k=K_HUBER,
                                                 differentiable=True, deterministic_backward=True)
            T = prov.localize(pc, live, prev)[:, 0]
            mask = prov.last_outlier_mask
        else:
            T, mask = composed(ops, pc, live, prev, RULE, weights=f(live), differentiable=True, deterministic=True, stride=2,
                               numiters=5, huber_k=K_HUBER)
        assert T.grad_fn is not None and not mask.requires_grad
        g = torch.autograd.grad(T, [vertex, prev, scale] + P + N, Tb)
        torch.cuda.synchronize()
        grads.append([host(T), host(mask)] + [host(x) for x in g])
    for i, (a, b) in enumerate(zip(*grads)):
        assert same(a, b), i
        assert i < 2 or np.abs(a).max() > 0, i
    assert grads[0][1].any()


# ------------------------------------------------------------------------------------------ 4. the driver
def test_pointfusion_keeps_the_outliers_out_of_the_map(gs, ops, sequences):
    from gradslam_amd.slam.fusionutils import update_map_fusion
    B, L = len(SEEDS), 4
    kw = dict(stride=2, numiters=6, huber_k=K_HUBER)
    # the hand-written loop: render / solve / mask / refine / masked map update
    frames = moved_frames(gs, sequences, first_pose_only=True)
    pc = gs.Pointclouds(device="cuda")
    prev, want, masks = None, [], []
    for s in range(L):
        live = frames[:, s]
        fused = live
        if s > 0:
            pose, mask = composed(ops, pc, live, prev, RULE, **kw)
            live.poses = pose.view(B, 1, 4, 4)
            masks.append(mask)
            d = live.depth_image.clone()
            d[:, 0, ..., 0][mask] = 0
            fused = gs.RGBDImages(live.rgb_image, d, live.intrinsics, live.poses)
        pc = update_map_fusion(pc, fused, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180), FUSION["sigma"],
                               inplace=True)
        prev = live.poses[:, 0].contiguous()
        want.append(prev.clone())
    want = torch.stack(want, 1)
    assert all(host(m).any() for m in masks)
    for inplace in (True, False):
        frames = moved_frames(gs, sequences, first_pose_only=True)
        before = frames.depth_image.clone()
        slam = gs.slam.PointFusion(odom="projicp", device="cuda", dsratio=2, numiters=6, huber_k=K_HUBER,
                                   odom_outlier_mask=RULE, fuse_outliers=False, **FUSION)
        got_pc = gs.Pointclouds(device="cuda")
        prv, got = None, []
        for s in range(L):
            live = frames[:, s]
            got_pc, poses = slam.step(got_pc, live, prv, inplace=inplace)
            assert same(live.poses, host(poses))                 # the pose is written back to the caller's frame
            if s > 0:
                assert same(slam.odomprov.last_outlier_mask, host(masks[s - 1])), s
            prv = live
            got.append(poses[:, 0].clone())
        assert same(torch.stack(got, 1), host(want)), inplace
        assert torch.equal(frames.depth_image, before)           # the caller's frames are unchanged
        for b in range(B):
            for g, x in zip(map_rows(got_pc, b), map_rows(pc, b)):
                assert same(g, x), (inplace, b)
    # fuse_outliers=True: the same poses for the first localisation, another map
    frames = moved_frames(gs, sequences, first_pose_only=True)
    slam = gs.slam.PointFusion(odom="projicp", device="cuda", dsratio=2, numiters=6, huber_k=K_HUBER, odom_outlier_mask=RULE,
                               **FUSION)
    all_pc, poses = slam(frames)
    assert same(poses[:, 1], host(want[:, 1])) and map_rows(all_pc, 0)[0].shape[0] > map_rows(pc, 0)[0].shape[0]
