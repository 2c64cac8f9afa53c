"""GPU tests of the projective-association ICP (gs_picp.hip -> gs_projective_icp_*_f32 -> ops.projective_icp* ->
ProjectiveICPOdometryProvider -> ICPSLAM / PointFusion with odom="projicp") against its NumPy restatement
(tests/picp_ref.py: the oracle's point transform, projection, similarity test and se3_exp, the 28 exact float64 terms,
the documented reduction order, the Gauss-Jordan solve in double).

Every operation of the kernels is restated in the same order, the reduction order is fixed and there are no atomics, so
every comparison is for EQUAL BITS (float32 as uint32, the float64 sums as uint64); the only tolerances are the two
distances to the ground truth that the CPU tests establish for the restatement (1e-3 m for one solve, 5 mm for the
6-frame loop)."""
import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from oracle import oracle as o
from tests import picp_ref as pr

pytestmark = pytest.mark.gpu

H, W, L = 60, 80, 6


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


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


def edge_fixture(h, w, stride):
    """The convergence fixture of size h x w, bent so that one linearisation at `T` meets every reject code: zeroed, NaN
    and negative depths (1); T = the ground truth pushed 4 cm along x, which carries a border column out of the model view
    (2); -1 holes, one entry = count and one = count + 5 in the index image, a device count 3 below the rows the render
    saw, in buffers 16 rows longer (3); one associated map point moved 0.2 m away (4); one associated normal flipped (5).
    Cached and read-only."""
    key = (h, w, stride)
    if key in _EDGE:
        return _EDGE[key]
    fx = dict(pr.convergence_fixture(h, w))
    n = fx["count"]
    count = n - 3
    depth = fx["depth"].copy()
    depth[::stride, ::stride][2, 3] = 0.0
    depth[::stride, ::stride][3, 5] = np.nan
    depth[::stride, ::stride][4, 2] = -1.0
    T = np.array(fx["gt"], np.float32)
    T[0, 3] += np.float32(0.04)
    P = np.zeros((n + 16, 3), np.float32)
    N = np.zeros((n + 16, 3), np.float32)
    P[:n], N[:n] = fx["points"], fx["normals"]
    P[n:] = np.nan                                  # rows beyond the count must never be read
    index = fx["index"].copy()
    fx.update(depth=depth, points=P, normals=N, index=index, count=count, T=T)
    r = pr.rows(*pr.args_of(fx), T, stride=stride)
    used = np.nonzero(r.code == 0)[0]
    assert used.size > 60
    far, flip = r.row[used[used.size // 3]], r.row[used[2 * used.size // 3]]
    assert far != flip
    P[far, 1] += np.float32(0.2)
    N[flip] = -N[flip]
    # index entries that slots of this lattice actually read: those of used slots
    pix = o.project_map(o.transform_points(
        np.ascontiguousarray(fx["vertex"][::stride, ::stride]).reshape(-1, 3), T), fx["model_pose"], fx["K"], h, w)
    hit = [int(pix[used[k]]) for k in (1, used.size // 5, used.size // 2, used.size - 2)]
    assert len(set(hit)) == 4
    flat = index.reshape(-1)
    flat[hit[0]], flat[hit[1]], flat[hit[2]], flat[hit[3]] = -1, -1, count, count + 5
    for val in fx.values():
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    _EDGE[key] = fx
    return fx


def hip_args(fx):
    """the positional tensors of ops.projective_icp / _rows up to the map normals, and the device count"""
    t = [dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals")]
    return t, torch.tensor([fx["count"]], dtype=torch.int64, device="cuda")


def same_solve(got, want, what=""):
    (T, trace), (rT, rtrace) = got, want
    T, trace = host(T), host(trace)
    assert np.array_equal(bits(T), bits(rT)), (what, T, rT)
    assert np.array_equal(bits(trace), bits(rtrace)), (what, trace, rtrace)


# ------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("h,w,stride", [(60, 80, 1), (60, 80, 4), (37, 53, 3), (37, 53, 1), (257, 257, 1),
                                        (363, 362, 1)])
def test_rows_bit_for_bit(ops, h, w, stride):
    """37 x 53 stride 3: a 13 x 18 lattice, 234 slots, one partial chunk; stride 1: 1 961 slots, 7 chunks and a tail of
    169; 257 x 257: 66 049 slots, 259 chunks, i.e. two tiles of the finish kernel's column sum, the second of 3 chunks,
    and a last chunk of one slot; 363 x 362: 131 406 slots, 514 chunks, three tiles (the prefetch is taken twice)"""
    fx = edge_fixture(h, w, stride)
    want = pr.rows(*pr.args_of(fx), fx["T"], stride=stride)
    assert set(np.unique(want.code)) == {0, 1, 2, 3, 4, 5}, np.bincount(want.code)
    assert (want.row[want.code == 3] >= fx["count"]).sum() >= 2 and (want.row[want.code == 3] == -1).sum() >= 1
    t, n_dev = hip_args(fx)
    got = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride)
    torch.cuda.synchronize()
    ns = want.code.shape[0]
    assert tuple(got.code.shape) == (ns,) and tuple(got.a.shape) == (ns, 6) and got.sums.dtype == torch.float64
    assert np.array_equal(host(got.code), want.code), np.nonzero(host(got.code) != want.code)
    assert np.array_equal(host(got.row), want.row)
    assert np.array_equal(bits(host(got.a)), bits(want.a))
    assert np.array_equal(bits(host(got.b)), bits(want.b))
    assert np.array_equal(bits(host(got.sums)), bits(want.sums)), (host(got.sums), want.sums)
    assert int(got.count) == want.count > 0
    assert np.isfinite(host(got.sums)).all()        # (the NaN rows beyond the count were not read)


# ------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("size,stride,numiters", [((60, 80), 1, 10), ((60, 80), 4, 10), ((257, 257), 1, 2)],
                         ids=["1", "4", "257x257-1"])
def test_solve_bit_for_bit_on_the_convergence_fixture(ops, size, stride, numiters):
    """257 x 257: 259 chunks, two tiles of the finish kernel's column sum, in a solve"""
    fx = pr.convergence_fixture(*size)
    want = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride, numiters=numiters)
    t = [dev(fx[k]) for k in pr.ARGS[:-1]]
    got = ops.projective_icp(*t, dev(fx["T0"]), stride=stride, numiters=numiters, return_trace=True)
    same_solve(got, want, "stride %d" % stride)
    again = ops.projective_icp(*t, dev(fx["T0"]), stride=stride, numiters=numiters, return_trace=True)
    assert np.array_equal(bits(host(got[0])), bits(host(again[0]))) and np.array_equal(bits(host(got[1])),
                                                                                        bits(host(again[1])))
    # against the ground truth: the bound the CPU test establishes for the restatement
    err = np.linalg.norm(host(got[0])[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    print("stride %d: HIP translation error %.3g m" % (stride, err))
    assert err <= 1e-3
    plain = ops.projective_icp(*t, dev(fx["T0"]), stride=stride, numiters=numiters)
    assert np.array_equal(bits(host(plain)), bits(host(got[0])))


@pytest.mark.parametrize("stride", [3, 1])
def test_solve_bit_for_bit_with_stale_entries_and_a_device_count(ops, stride):
    fx = edge_fixture(37, 53, stride)
    want = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride, numiters=6)
    t, n_dev = hip_args(fx)
    got = ops.projective_icp(*t, dev(fx["T0"]), n_dev=n_dev, stride=stride, numiters=6, return_trace=True)
    same_solve(got, want, "37x53 stride %d" % stride)
    again = ops.projective_icp(*t, dev(fx["T0"]), n_dev=n_dev, stride=stride, numiters=6, return_trace=True)
    assert np.array_equal(bits(host(got[0])), bits(host(again[0])))
    assert np.isfinite(host(got[0])).all() and host(got[1])[-1, 0] > 20


# ------------------------------------------------------------------------------------------ batch
def three_sequences():
    """same image size, different frames, scenes and map sizes (the third map also behind a device count)"""
    a = dict(pr.convergence_fixture(H, W, 5, "wave"))
    b = dict(pr.convergence_fixture(H, W, 3, "facets"))
    c = dict(edge_fixture(H, W, 4))
    keep = b["count"] - 400            # a shorter map under the same index image: its last 400 rows are stale entries
    b.update(points=b["points"][:keep], normals=b["normals"][:keep], count=keep)
    a["n_dev"], b["n_dev"], c["n_dev"] = None, None, c["count"]
    assert len({x["points"].shape[0] for x in (a, b, c)}) == 3
    return [a, b, c]


def batch_call(ops, seqs, **kw):
    st = lambda k: torch.stack([dev(q[k]) for q in seqs])   # noqa: E731
    maps = [(dev(q["points"]), dev(q["normals"]), None, None, None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in seqs]
    return ops.projective_icp_batch(st("vertex"), st("normal"), st("depth"), st("K"), st("index"), st("model_pose"), maps,
                                    st("T0"), return_trace=True, **kw)


def single_call(ops, q, **kw):
    t = [dev(q[k]) for k in pr.ARGS[:-1]]
    n_dev = None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")
    return ops.projective_icp(*t, dev(q["T0"]), n_dev=n_dev, return_trace=True, **kw)


def test_batch_of_three_equals_three_single_calls(ops):
    seqs = three_sequences()
    kw = dict(stride=2, numiters=5)
    T, trace = batch_call(ops, seqs, **kw)
    assert tuple(T.shape) == (3, 4, 4) and tuple(trace.shape) == (3, 5, 8)
    for b, q in enumerate(seqs):
        sT, strace = single_call(ops, q, **kw)
        assert np.array_equal(bits(host(T[b])), bits(host(sT))), b
        assert np.array_equal(bits(host(trace[b])), bits(host(strace))), b
    want = pr.solve(*pr.args_of(seqs[1]), seqs[1]["T0"], **kw)
    same_solve((T[1], trace[1]), want, "facets")
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
        sT, _ = single_call(ops, seqs[b], **kw)
        assert np.array_equal(bits(host(T[b])), bits(host(sT))), b
    assert (host(trace)[:, -1, 0] > 20).all()


# ------------------------------------------------------------------------------------------ degenerate
@pytest.mark.parametrize("what", ["no_winner", "no_depth"])
def test_no_inlier_returns_the_initial_pose_bits(ops, what):
    fx = dict(pr.convergence_fixture())
    if what == "no_winner":
        fx["index"] = np.full_like(fx["index"], -1)
    else:
        fx["depth"] = np.zeros_like(fx["depth"])
    T0 = np.array(fx["T0"], np.float32)
    T0[2, 0] = -0.0                     # a product with the identity would turn it into +0
    t = [dev(fx[k]) for k in pr.ARGS[:-1]]
    T, trace = ops.projective_icp(*t, dev(T0), stride=1, numiters=3, return_trace=True)
    assert np.array_equal(bits(host(T)), bits(T0))
    assert (host(trace) == 0).all() and np.isfinite(host(T)).all()
    r = ops.projective_icp_rows(*t, dev(T0))
    assert int(r.count) == 0 and (host(r.sums) == 0).all() and not (host(r.code) == 0).any()


# ------------------------------------------------------------------------------------------ drivers
SEEDS = (0, 1)
KW = dict(dsratio=2, numiters=10)
FUSION = dict(dist_th=0.05, angle_th=20, sigma=0.6)


@pytest.fixture(scope="module")
def sequences():
    return [make_sequence(L, H, W, seed=s) for s in SEEDS]


def frames_of(gs, sequences, first_pose_only=True):
    st = lambda k: torch.from_numpy(np.stack([q[k] for q in sequences])).cuda()   # noqa: E731
    poses = st("poses")
    if first_pose_only:
        poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)


def map_rows(pc, b):
    return [host(t[b]) for t in (pc.points_list, pc.normals_list, pc.colors_list)] + \
        ([host(pc.features_list[b])] if pc.has_features else [])


def hand_written_loop(gs, ops, which, frames, prune=None, **kw):
    """render the map at the previous pose, solve from that pose, update the map: the calls a user would make"""
    import math
    from gradslam_amd.slam.fusionutils import update_map_aggregate, update_map_fusion
    B = frames.shape[0]
    pc = gs.Pointclouds(device="cuda")
    out = []
    prev = None
    K = frames.intrinsics[:, 0].contiguous()
    for s in range(L):
        live = frames[:, s]
        if s > 0:
            maps = [(pc._buf["points"][b], pc._buf["normals"][b], None, None) + tuple(pc._count_of(b)) for b in range(B)]
            if which == "PointFusion":
                _, extras = pc.render(frames.intrinsics, prev.view(B, 1, 4, 4), H, W, return_extras=True)
                index = extras["index"][:, 0]
            else:       # (the aggregate map has no confidence channel: Pointclouds.render asks for a surfel map)
                index = ops.render_map_batch(maps, prev.view(B, 1, 4, 4), K, H, W).index[:, 0]
            fr = live.to_channels_last()
            pose = ops.projective_icp_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K,
                                            index, prev, maps, prev, **kw)
            live.poses = pose.view(B, 1, 4, 4)
        if which == "PointFusion":
            pc = update_map_fusion(pc, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180),
                                   FUSION["sigma"], inplace=True)
        else:
            pc = update_map_aggregate(pc, live, inplace=True)
        prev = live.poses[:, 0].contiguous()
        out.append(prev.clone())
    return pc, torch.stack(out, 1)


def run_steps(slam, gs, frames, inplace):
    pc = gs.Pointclouds(device="cuda")
    prev, out = None, []
    for s in range(L):
        live = frames[:, s]
        pc, poses = slam.step(pc, live, prev, inplace=inplace)
        live.poses = poses
        prev = live
        out.append(poses[:, 0].clone())
    return pc, torch.stack(out, 1)


def make_slam(gs, which, **extra):
    cls = getattr(gs.slam, which)
    kw = dict(KW, odom="projicp", device="cuda", **extra)
    if which == "PointFusion":
        kw.update(FUSION)
    return cls(**kw)


@pytest.fixture(scope="module")
def by_hand(gs, ops, sequences):
    res = {}
    for which in ("PointFusion", "ICPSLAM"):
        pc, poses = hand_written_loop(gs, ops, which, frames_of(gs, sequences), stride=KW["dsratio"],
                                      numiters=KW["numiters"])
        res[which] = ([map_rows(pc, b) for b in range(len(SEEDS))], host(poses))
    return res


@pytest.mark.parametrize("how", ["step_inplace", "step_out_of_place", "forward"])
@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_equal_the_hand_written_loop(gs, sequences, by_hand, which, how):
    slam = make_slam(gs, which)
    frames = frames_of(gs, sequences)
    if how == "forward":
        pc, poses = slam(frames)
    else:
        pc, poses = run_steps(slam, gs, frames, inplace=how == "step_inplace")
    want_maps, want_poses = by_hand[which]
    poses = host(poses)
    assert np.array_equal(bits(poses), bits(want_poses)), np.abs(poses - want_poses).max()
    for b in range(len(SEEDS)):
        for got, want in zip(map_rows(pc, b), want_maps[b]):
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (b, got.shape, want.shape)
        err = np.linalg.norm(poses[b, -1, :3, 3].astype(np.float64) - sequences[b]["poses"][-1, :3, 3])
        print("%s %s seed %d: last pose %.3g m from the ground truth" % (which, how, SEEDS[b], err))
        assert err <= 5e-3
    assert not np.array_equal(poses[:, 1], poses[:, 0])


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_depth_filter_equals_prefiltered_frames(gs, sequences, which):
    flt = dict(radius=2, sigma_space=1.5, sigma_range=0.05)
    pc_a, poses_a = make_slam(gs, which, depth_filter=flt)(frames_of(gs, sequences))
    pc_b, poses_b = make_slam(gs, which)(frames_of(gs, sequences).bilateral_filter(**flt))
    plain = make_slam(gs, which)(frames_of(gs, sequences))[1]
    assert np.array_equal(bits(host(poses_a)), bits(host(poses_b)))
    assert not np.array_equal(host(poses_a), host(plain))
    for b in range(len(SEEDS)):
        for got, want in zip(map_rows(pc_a, b), map_rows(pc_b, b)):
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), b


def test_pruning_between_frames(gs, ops, sequences):
    """a prune after every step: the next localisation renders its index image from the compacted map (a stale index
    would point past the new count or at another surfel)"""
    slam = make_slam(gs, "PointFusion", prune_min_confidence=1.5, prune_min_age=1, prune_every=1)
    frames = frames_of(gs, sequences)
    pc, poses = run_steps(slam, gs, frames, inplace=True)
    full, _ = run_steps(make_slam(gs, "PointFusion"), gs, frames_of(gs, sequences), inplace=True)
    poses = host(poses)
    assert np.isfinite(poses).all()
    B = len(SEEDS)
    for b in range(B):
        assert 0 < pc.points_list[b].shape[0] < full.points_list[b].shape[0]
        err = np.linalg.norm(poses[b, -1, :3, 3].astype(np.float64) - sequences[b]["poses"][-1, :3, 3])
        print("pruned run, seed %d: last pose %.3g m from the ground truth" % (SEEDS[b], err))
    # the provider against the pruned map == render + solve by hand on that map
    live = frames_of(gs, sequences)[:, L - 1]
    prev = torch.from_numpy(poses[:, L - 2]).cuda()
    got = slam.odomprov.localize(pc, live, prev.view(B, 1, 4, 4))
    maps = [(pc._buf["points"][b], pc._buf["normals"][b], None, None) + tuple(pc._count_of(b)) for b in range(B)]
    _, extras = pc.render(live.intrinsics, prev.view(B, 1, 4, 4), H, W, return_extras=True)
    n = [int(pc.points_list[b].shape[0]) for b in range(B)]
    assert all(int(extras["index"][b].max()) < n[b] for b in range(B))
    fr = live.to_channels_last()
    want = ops.projective_icp_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0],
                                    live.intrinsics[:, 0].contiguous(), extras["index"][:, 0], prev, maps, prev,
                                    stride=KW["dsratio"], numiters=KW["numiters"])
    assert tuple(got.shape) == (B, 1, 4, 4) and np.array_equal(bits(host(got[:, 0])), bits(host(want)))


def test_unknown_odometry_still_raises_and_grad_inputs_warn(gs, ops, sequences):
    with pytest.raises(ValueError, match="not supported"):
        gs.slam.PointFusion(odom="projective")
    with pytest.raises(ValueError, match="not supported"):
        gs.slam.ICPSLAM(odom="picp")
    fx = pr.convergence_fixture()
    t = [dev(fx[k]) for k in pr.ARGS[:-1]]
    t[0].requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        T = ops.projective_icp(*t, dev(fx["T0"]), stride=4, numiters=2)
    assert not T.requires_grad
