"""GPU tests of the projective ICP's colour term (gs_picp_color.hip -> gs_model_intensity_f32 /
gs_projective_icp_color_*_f32 -> ops.model_intensity / projective_icp_color* -> ProjectiveICPOdometryProvider(color_weight)
-> ICPSLAM / PointFusion(odom="projicp", color_weight=...)) against its NumPy restatement (tests/picp_color_ref.py).

Every operation is restated in the same order, the reduction order is fixed and there are no atomics: every comparison is
for EQUAL BITS.  The only tolerances are distances to the ground truth that the CPU tests establish for the restatement
(2.5 mm and 1e-3 m for one solve, 5 mm for the 6-frame loop)."""
import math

import numpy as np
import pytest
import torch

from tests import picp_color_ref as pc
from tests import picp_ref as pr
from tests.test_hip_picp import FUSION, bits, dev, edge_fixture, host

pytestmark = pytest.mark.gpu

H, W, L = 60, 80, 6
WEIGHT = 0.2


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


# ------------------------------------------------------------------------------------------ fixtures
_EDGE = {}


def color_edge_fixture(h, w, stride):
    """tests.test_hip_picp.edge_fixture (every reject code, stale index entries, a device count below the buffers' rows) on
    the textured "wave" sequence -- the same depths, hence the same geometry -- with the live colour and the model
    intensity of the view's colour image under the BENT index image.  Cached and read-only."""
    key = (h, w, stride)
    if key not in _EDGE:
        fx = dict(edge_fixture(h, w, stride))
        tf = pc.textured_fixture(h, w, scene="wave")
        assert np.array_equal(tf["depth"], pr.convergence_fixture(h, w)["depth"])
        fx.update(color=tf["color"], model=pc.model_intensity(tf["view_color"], fx["index"]), n_dev=fx["count"])
        fx["model"].setflags(write=False)
        _EDGE[key] = fx
    return _EDGE[key]


def hip_args(fx):
    """(the positional tensors up to the map normals, those after the pose, the device count)"""
    t = [dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals")]
    n_dev = None if fx.get("n_dev") is None else torch.tensor([fx["n_dev"]], dtype=torch.int64, device="cuda")
    return t, [dev(fx["color"]), dev(fx["model"])], n_dev


def solve_hip(ops, fx, T0=None, weight=WEIGHT, **kw):
    t, c, n_dev = hip_args(fx)
    return ops.projective_icp_color(*t, dev(fx["T0"] if T0 is None else T0), *c, color_weight=weight, n_dev=n_dev,
                                    return_trace=True, **kw)


def same_solve(got, want, what=""):
    (T, trace), (rT, rtrace) = got, want
    T, trace = host(T), host(trace)
    assert np.array_equal(bits(T), bits(rT)), (what, T, rT)
    assert np.array_equal(bits(trace), bits(rtrace)), (what, trace, rtrace)


# ------------------------------------------------------------------------------------------ model intensity
@pytest.mark.parametrize("h,w", [(60, 80), (37, 53)])
def test_model_intensity_bit_for_bit(ops, h, w):
    """37 x 53: neither a multiple of the 8-row nor of the 32-column tile; two views in one call (the grid's z extent);
    holes of the render, plus holes on the border, next to it and in a corner"""
    views = []
    for scene in ("wave", "plane"):
        fx = pc.textured_fixture(h, w, scene=scene)
        index = fx["index"].copy()
        for (a, b) in ((0, 5), (1, 7), (h - 1, w - 1), (h - 2, 3), (9, 0), (11, w - 2), (8, 31), (8, 32)):
            index[a, b] = -1
        views.append((fx["view_color"], index))
    want = np.stack([pc.model_intensity(c, i) for c, i in views])
    assert (want[..., 3] == 1).any() and (want[:, 1, 6, 3] == 0).all() and (want[:, 2, 7, 3] == 0).all()
    color, index = dev(np.stack([c for c, _ in views])), dev(np.stack([i for _, i in views]))
    got = ops.model_intensity(color, index)
    assert tuple(got.shape) == (2, h, w, 4)
    assert np.array_equal(bits(host(got)), bits(want))
    one = ops.model_intensity(color[1], index[1])
    assert np.array_equal(bits(host(one)), bits(want[1]))
    assert np.array_equal(bits(host(ops.model_intensity(color, index))), bits(host(got)))


# ------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("h,w,stride", [(60, 80, 1), (60, 80, 4), (37, 53, 3), (37, 53, 1), (257, 257, 1)])
def test_rows_bit_for_bit(ops, h, w, stride):
    """257 x 257: 259 chunks, two tiles of the finish kernel's column sum"""
    fx = color_edge_fixture(h, w, stride)
    want = pc.rows(*pc.args_of(fx), fx["T"], WEIGHT, stride=stride)
    assert set(np.unique(want.code)) == {0, 1, 2, 3, 4, 5}, np.bincount(want.code)
    # every colour outcome: used, geometric reject, used without a colour row (ok = 0)
    assert want.colored.sum() > 20 and ((want.code == 0) & ~want.colored).sum() > 5 and (want.code != 0).sum() > 5
    t, c, n_dev = hip_args(fx)
    got = ops.projective_icp_color_rows(*t, dev(fx["T"]), *c, color_weight=WEIGHT, n_dev=n_dev, stride=stride)
    torch.cuda.synchronize()
    ns = want.code.shape[0]
    assert tuple(got.code.shape) == (ns,) and tuple(got.ac.shape) == (ns, 6) and got.sums.dtype == torch.float64
    assert np.array_equal(host(got.code), want.code), np.nonzero(host(got.code) != want.code)
    assert np.array_equal(host(got.row), want.row)
    assert np.array_equal(host(got.colored) == 1, want.colored)
    for name in ("a", "b", "ac", "bc", "sums"):
        assert np.array_equal(bits(host(getattr(got, name))), bits(getattr(want, name))), name
    assert int(got.count) == want.count > 0 and int(got.color_count) == want.color_count > 0
    assert np.isfinite(host(got.sums)).all()        # (the NaN rows beyond the count were not read)
    # the geometric part is the plain call's
    plain = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride)
    assert np.array_equal(host(plain.code), host(got.code)) and np.array_equal(bits(host(plain.a)), bits(host(got.a)))
    assert not np.array_equal(host(plain.sums), host(got.sums))


# ------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("scene,size,stride,numiters",
                         [("plane", (60, 80), 1, 10), ("wave", (60, 80), 1, 10), ("plane", (60, 80), 4, 10),
                          ("wave", (60, 80), 4, 10), ("wave", (257, 257), 1, 2)],
                         ids=["1-plane", "1-wave", "4-plane", "4-wave", "257x257-1-wave"])
def test_solve_bit_for_bit(ops, scene, size, stride, numiters):
    """257 x 257: 259 chunks, two tiles of the finish kernel's column sum, in a solve"""
    fx = pc.textured_fixture(*size, scene=scene)
    want = pc.solve(*pc.args_of(fx), fx["T0"], WEIGHT, stride=stride, numiters=numiters)
    got = solve_hip(ops, fx, stride=stride, numiters=numiters)
    same_solve(got, want, "%s stride %d" % (scene, stride))
    again = solve_hip(ops, fx, stride=stride, numiters=numiters)    # two calls give identical bits
    assert np.array_equal(bits(host(got[0])), bits(host(again[0]))) and np.array_equal(bits(host(got[1])),
                                                                                        bits(host(again[1])))
    t, c, _ = hip_args(fx)
    no_trace = ops.projective_icp_color(*t, dev(fx["T0"]), *c, color_weight=WEIGHT, stride=stride, numiters=numiters)
    assert np.array_equal(bits(host(no_trace)), bits(host(got[0])))


def test_the_colour_term_pins_the_plane(ops):
    """the CPU test's claim on the GPU: 15 iterations from 25 mm off; geometry alone ends farther away than it started,
    the joint solve within a tenth of the start error; on "wave" it stays within 1e-3 m"""
    fx = pc.textured_fixture(scene="plane")
    start = np.linalg.norm(fx["T0"][:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    t, c, _ = hip_args(fx)
    Tg = ops.projective_icp(*t, dev(fx["T0"]), stride=1, numiters=15)
    Tc, _ = solve_hip(ops, fx, stride=1, numiters=15)
    eg = np.linalg.norm(host(Tg)[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    ec = np.linalg.norm(host(Tc)[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    print("plane: start %.4g m, geometry only %.4g m, colour weight %.2g: %.4g m" % (start, eg, WEIGHT, ec))
    assert eg > start and ec <= 0.1 * start
    fw = pc.textured_fixture(scene="wave")
    Tw, _ = solve_hip(ops, fw, stride=1, numiters=15)
    ew = np.linalg.norm(host(Tw)[:3, 3].astype(np.float64) - fw["gt"][:3, 3])
    print("wave: colour weight %.2g: %.4g m" % (WEIGHT, ew))
    assert ew <= 1e-3


@pytest.mark.parametrize("stride", [3, 1])
def test_solve_with_stale_entries_and_a_device_count(ops, stride):
    """the index image points past the device count (as after a prune that shortened the map): never dereferenced"""
    fx = color_edge_fixture(37, 53, stride)
    want = pc.solve(*pc.args_of(fx), fx["T0"], WEIGHT, stride=stride, numiters=6)
    got = solve_hip(ops, fx, stride=stride, numiters=6)
    same_solve(got, want, "37x53 stride %d" % stride)
    assert np.isfinite(host(got[0])).all() and host(got[1])[-1, 0] > 20 and host(got[1])[-1, 8] > 5


def test_weight_zero_returns_the_plain_pose_bits(ops):
    fx = pc.textured_fixture(scene="wave")
    t, c, _ = hip_args(fx)
    for stride in (1, 4):
        T, trace = solve_hip(ops, fx, weight=0.0, stride=stride, numiters=6)
        pT, ptrace = ops.projective_icp(*t, dev(fx["T0"]), stride=stride, numiters=6, return_trace=True)
        assert np.array_equal(bits(host(T)), bits(host(pT)))
        assert np.array_equal(bits(host(trace)[:, :8]), bits(host(ptrace))) and (host(trace)[:, 8] > 100).all()


def test_a_view_without_any_ok_pixel_returns_the_plain_bits(ops):
    fx = dict(pc.textured_fixture(scene="wave"))
    model = fx["model"].copy()
    model[..., 1:] = 0.0                       # ok = 0 everywhere (and no gradient, as the pre-pass would write)
    fx["model"] = model
    t, c, _ = hip_args(fx)
    T, trace = solve_hip(ops, fx, stride=2, numiters=5)
    pT, ptrace = ops.projective_icp(*t, dev(fx["T0"]), stride=2, numiters=5, return_trace=True)
    assert np.array_equal(bits(host(T)), bits(host(pT)))
    assert np.array_equal(bits(host(trace)[:, :8]), bits(host(ptrace))) and (host(trace)[:, 8] == 0).all()


@pytest.mark.parametrize("what", ["no_winner", "no_depth"])
def test_no_geometric_inlier_returns_the_initial_pose_bits(ops, what):
    fx = dict(pc.textured_fixture(scene="plane"))
    if what == "no_winner":
        fx["index"] = np.full_like(fx["index"], -1)       # (the model intensity keeps its ok pixels: no row reaches them)
    else:
        fx["depth"] = np.zeros_like(fx["depth"])
    T0 = np.array(fx["T0"], np.float32)
    T0[2, 0] = -0.0                     # a product with the identity would turn it into +0
    T, trace = solve_hip(ops, fx, T0=T0, stride=1, numiters=3)
    assert np.array_equal(bits(host(T)), bits(T0))
    assert (host(trace) == 0).all() and np.isfinite(host(T)).all()


# ------------------------------------------------------------------------------------------ batch
def three_sequences():
    """same image size, different scenes, frames and map sizes (the third behind a device count, with stale entries)"""
    a = dict(pc.textured_fixture(H, W, 5, "plane"))
    b = dict(pc.textured_fixture(H, W, 3, "tilted"))
    c = dict(color_edge_fixture(H, W, 4))
    keep = b["count"] - 400            # a shorter map under the same index image: its last 400 rows are stale entries
    b.update(points=b["points"][:keep], normals=b["normals"][:keep], count=keep)
    a["n_dev"], b["n_dev"] = None, None
    assert len({x["points"].shape[0] for x in (a, b, c)}) == 3
    return [a, b, c]


def batch_call(ops, seqs, **kw):
    st = lambda k: torch.stack([dev(q[k]) for q in seqs])   # noqa: E731
    maps = [(dev(q["points"]), dev(q["normals"]), None, None, None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in seqs]
    return ops.projective_icp_color_batch(st("vertex"), st("normal"), st("depth"), st("K"), st("index"),
                                          st("model_pose"), maps, st("T0"), st("color"), st("model"),
                                          color_weight=WEIGHT, return_trace=True, **kw)


def test_batch_of_three_equals_three_single_calls(ops):
    seqs = three_sequences()
    kw = dict(stride=2, numiters=5)
    T, trace = batch_call(ops, seqs, **kw)
    assert tuple(T.shape) == (3, 4, 4) and tuple(trace.shape) == (3, 5, 9)
    for b, q in enumerate(seqs):
        sT, strace = solve_hip(ops, q, **kw)
        assert np.array_equal(bits(host(T[b])), bits(host(sT))), b
        assert np.array_equal(bits(host(trace[b])), bits(host(strace))), b
    want = pc.solve(*pc.args_of(seqs[1]), seqs[1]["T0"], WEIGHT, **kw)
    same_solve((T[1], trace[1]), want, "tilted")
    assert len({host(T[b]).tobytes() for b in range(3)}) == 3


def test_batch_of_nine_crosses_the_launch_boundary(ops):
    """8 sequences per launch: the ninth goes through a launch of its own"""
    seqs = three_sequences()
    kw = dict(stride=4, numiters=4)
    T, trace = batch_call(ops, [seqs[i % 3] for i in range(9)], **kw)
    for i in range(9):
        assert np.array_equal(bits(host(T[i])), bits(host(T[i % 3]))), i
        assert np.array_equal(bits(host(trace[i])), bits(host(trace[i % 3]))), i
    for b in range(3):
        sT, _ = solve_hip(ops, seqs[b], **kw)
        assert np.array_equal(bits(host(T[b])), bits(host(sT))), b
    assert (host(trace)[:, -1, 0] > 20).all() and (host(trace)[:, -1, 8] > 5).all()


# ------------------------------------------------------------------------------------------ drivers
SCENES = ("plane", "wave")
KW = dict(dsratio=2, numiters=10)
DRIVER_WEIGHT = 1.0     # (tests/test_picp_color_cpu.py: the weight at which the restated loop stays within 5 mm on "plane")


def frames_of(gs, first_pose_only=True):
    seqs = [pc.textured_sequence(L, H, W, s) for s in SCENES]
    st = lambda k: torch.from_numpy(np.stack([q[k] for q in seqs])).cuda()   # noqa: E731
    poses = st("poses")
    if first_pose_only:
        poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)


def map_rows(pc_, b):
    return [host(t[b]) for t in (pc_.points_list, pc_.normals_list, pc_.colors_list)] + \
        ([host(pc_.features_list[b])] if pc_.has_features else [])


def hand_written_loop(gs, ops, which, frames, weight, prune_every=None):
    """render the map (index and colour) at the previous pose, build the model intensity, solve from that pose with the
    live colour, update the map: the calls a user would make"""
    from gradslam_amd.slam.fusionutils import update_map_aggregate, update_map_fusion
    B = frames.shape[0]
    m = gs.Pointclouds(device="cuda")
    out, prev = [], None
    K = frames.intrinsics[:, 0].contiguous()
    for s in range(L):
        live = frames[:, s]
        if s > 0:
            counts = [tuple(m._count_of(b)) for b in range(B)]
            view = ops.render_map_batch([(m._buf["points"][b], None, m._buf["colors"][b], None) + counts[b]
                                         for b in range(B)], prev.view(B, 1, 4, 4), K, H, W)
            model = ops.model_intensity(view.color[:, 0], view.index[:, 0])
            fr = live.to_channels_last()
            maps = [(m._buf["points"][b], m._buf["normals"][b], None, None) + counts[b] for b in range(B)]
            pose = ops.projective_icp_color_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0],
                                                  K, view.index[:, 0], prev, maps, prev, fr.rgb_image[:, 0], model,
                                                  color_weight=weight, stride=KW["dsratio"], numiters=KW["numiters"])
            live.poses = pose.view(B, 1, 4, 4)
        if which == "PointFusion":
            m = update_map_fusion(m, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180),
                                  FUSION["sigma"], inplace=True)
        else:
            m = update_map_aggregate(m, live, inplace=True)
        prev = live.poses[:, 0].contiguous()
        out.append(prev.clone())
    return m, torch.stack(out, 1)


def run_steps(slam, gs, frames, inplace):
    m = gs.Pointclouds(device="cuda")
    prev, out = None, []
    for s in range(L):
        live = frames[:, s]
        m, poses = slam.step(m, live, prev, inplace=inplace)
        live.poses = poses
        prev = live
        out.append(poses[:, 0].clone())
    return m, torch.stack(out, 1)


def make_slam(gs, which, **extra):
    kw = dict(KW, odom="projicp", device="cuda", **extra)
    if which == "PointFusion":
        kw.update(FUSION)
    return getattr(gs.slam, which)(**kw)


@pytest.fixture(scope="module")
def by_hand(gs, ops):
    res = {}
    for which in ("PointFusion", "ICPSLAM"):
        m, poses = hand_written_loop(gs, ops, which, frames_of(gs), DRIVER_WEIGHT)
        res[which] = ([map_rows(m, b) for b in range(len(SCENES))], host(poses))
    return res


@pytest.mark.parametrize("how", ["step_inplace", "forward"])
@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_equal_the_hand_written_loop(gs, by_hand, which, how):
    slam = make_slam(gs, which, color_weight=DRIVER_WEIGHT)
    frames = frames_of(gs)
    if how == "forward":
        m, poses = slam(frames)
    else:
        m, poses = run_steps(slam, gs, frames, inplace=True)
    want_maps, want_poses = by_hand[which]
    poses = host(poses)
    assert np.array_equal(bits(poses), bits(want_poses)), np.abs(poses - want_poses).max()
    for b in range(len(SCENES)):
        for got, want in zip(map_rows(m, b), want_maps[b]):
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (b, got.shape, want.shape)
    assert not np.array_equal(poses[:, 1], poses[:, 0])


def test_out_of_place_steps_filter_and_prune_schedule_run_with_the_weight(gs, by_hand):
    """step out of place gives the in-place bits; depth_filter= and the prune schedule go through the same provider"""
    frames = frames_of(gs)
    _, poses = run_steps(make_slam(gs, "PointFusion", color_weight=DRIVER_WEIGHT), gs, frames, inplace=False)
    assert np.array_equal(bits(host(poses)), bits(by_hand["PointFusion"][1]))
    flt = dict(radius=2, sigma_space=1.5, sigma_range=0.05)
    _, pa = make_slam(gs, "PointFusion", color_weight=DRIVER_WEIGHT, depth_filter=flt)(frames_of(gs))
    _, pb = make_slam(gs, "PointFusion", color_weight=DRIVER_WEIGHT)(frames_of(gs).bilateral_filter(**flt))
    assert np.array_equal(bits(host(pa)), bits(host(pb)))
    slam = make_slam(gs, "PointFusion", color_weight=DRIVER_WEIGHT, prune_min_confidence=1.5, prune_min_age=1,
                     prune_every=1)
    m, pp = run_steps(slam, gs, frames_of(gs), inplace=True)
    assert np.isfinite(host(pp)).all() and not np.array_equal(host(pp), by_hand["PointFusion"][1])
    # the provider against the pruned map (device-side count, compacted rows) == the calls by hand on that map
    B = len(SCENES)
    live = frames_of(gs)[:, L - 1]
    prev = pp[:, L - 2].contiguous()
    got = slam.odomprov.localize(m, live, prev.view(B, 1, 4, 4))
    from gradslam_amd import ops
    counts = [tuple(m._count_of(b)) for b in range(B)]
    K = live.intrinsics[:, 0].contiguous()
    view = ops.render_map_batch([(m._buf["points"][b], None, m._buf["colors"][b], None) + counts[b] for b in range(B)],
                                prev.view(B, 1, 4, 4), K, H, W)
    fr = live.to_channels_last()
    maps = [(m._buf["points"][b], m._buf["normals"][b], None, None) + counts[b] for b in range(B)]
    want = ops.projective_icp_color_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K,
                                          view.index[:, 0], prev, maps, prev, fr.rgb_image[:, 0],
                                          ops.model_intensity(view.color[:, 0], view.index[:, 0]),
                                          color_weight=DRIVER_WEIGHT, stride=KW["dsratio"], numiters=KW["numiters"])
    assert np.array_equal(bits(host(got[:, 0])), bits(host(want)))


def test_the_driver_with_the_weight_tracks_the_plane_and_without_it_does_not(gs, by_hand):
    gt = pc.textured_sequence(L, H, W, "plane")["poses"]
    with_w = by_hand["PointFusion"][1][0]
    _, plain = make_slam(gs, "PointFusion")(frames_of(gs))
    e_w = np.linalg.norm(with_w[-1, :3, 3].astype(np.float64) - gt[-1, :3, 3])
    e_p = np.linalg.norm(host(plain)[0, -1, :3, 3].astype(np.float64) - gt[-1, :3, 3])
    print("plane, PointFusion, last pose: %.4g m with color_weight %.2g, %.4g m without" % (e_w, DRIVER_WEIGHT, e_p))
    assert e_w <= 5e-3 < e_p


def test_a_map_without_colours_and_other_odometries_raise(gs, ops):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    frames = frames_of(gs)
    m, _ = make_slam(gs, "PointFusion")(frames[:, :2])
    bare = gs.Pointclouds(points=[p for p in m.points_list], normals=[n for n in m.normals_list])
    with pytest.raises(ValueError, match="colours"):
        ProjectiveICPOdometryProvider(color_weight=0.1).localize(bare, frames[:, 2], frames.poses[:, :1])
    with pytest.raises(ValueError, match="color_weight"):
        gs.slam.PointFusion(odom="gradicp", color_weight=0.1)
    fx = pc.textured_fixture(scene="plane")
    t, c, _ = hip_args(fx)
    with pytest.raises(ValueError, match="model_intensity"):
        ops.projective_icp_color(*t, dev(fx["T0"]), c[0], c[1][..., :3].contiguous(), color_weight=0.1)
