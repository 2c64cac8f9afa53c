"""GPU tests of the projective ICP's Huber weights (the *_robust_* entry points of gs_picp.hip, gs_picp_color.hip and
gs_picp_bwd.hip -> ops.projective_icp*(huber_delta=..., color_huber_delta=...) -> ProjectiveICPOdometryProvider ->
ICPSLAM / PointFusion(odom="projicp", huber_delta=...)).

Forward: every operation is restated in the same order by tests/picp_robust_ref.py, the reduction order is fixed and there
are no atomics, so every comparison is for EQUAL BITS.  Backward: the arbiter is the float64 NumPy adjoint of the same
file at the forward's float32 poses; a kernel output may differ from it by kernel_bound(gap) of tests/backward_cases.py,
the gap being the float32-vs-float64 distance of that NumPy adjoint (tests/picp_robust_backward_cases.py; no bound comes
from a kernel's output).  vertex_bar and init_pose_bar are compared for equal bits across runs."""
import math

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_color_ref as pcr
from tests import picp_ref as pr
from tests import picp_robust_backward_cases as rc
from tests import picp_robust_ref as rr
from tests.test_hip_picp import FUSION, bits, dev, edge_fixture, frames_of, host, map_rows
from tests.test_hip_picp_color import color_edge_fixture

pytestmark = pytest.mark.gpu

H, W, L = 60, 80, 4
DELTA, COLOR_DELTA, WEIGHT = 0.005, 0.02, 0.2
MAP_BOUND = bc.kernel_bound(0.0)    # two runs of the same float64 atomic sums, rounded once: float32 ulps of the scale


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


def geo(fx):
    """the positional tensors up to the map normals, and the device count (None: the bound is exact)"""
    t = [dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals")]
    n = fx["count"] if fx["count"] < fx["points"].shape[0] else None
    return t, None if n is None else torch.tensor([n], dtype=torch.int64, device="cuda")


def fixture(h, w, stride):
    """37 x 53: the edge fixture (every reject code, stale entries, a device count), linearised 4 cm off; 60 x 80: the
    convergence fixture with the moved block"""
    if (h, w) == (37, 53):
        return dict(edge_fixture(h, w, stride))
    fx = rr.moved_block(pr.convergence_fixture(h, w))
    fx["T"] = fx["T0"]
    return fx


def color_fixture(h, w, stride):
    if (h, w) == (37, 53):
        return dict(color_edge_fixture(h, w, stride))
    fx = rr.moved_block(pcr.textured_fixture(h, w, scene="plane"))
    fx["T"] = fx["T0"]
    return fx


def same_solve(got, want, what=""):
    (T, trace), (rT, rtrace) = got, want
    T, trace = host(T), host(trace)
    assert np.array_equal(bits(T), bits(rT)), (what, T, rT)
    assert np.array_equal(bits(trace), bits(rtrace)), (what, trace, rtrace)


SIZES = [(37, 53, 1), (37, 53, 3), (60, 80, 1), (60, 80, 4), (257, 257, 1)]   # (257 x 257: 259 chunks, two finish tiles)


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("h,w,stride", SIZES)
def test_solve_bit_for_bit(ops, h, w, stride):
    """37 x 53 stride 3: 234 slots, one partial chunk; stride 1: 7 chunks and a tail, both behind a device count;
    60 x 80: 19 and 2 chunks.  The taped forward and the delta = 0 keyword give the bits they must."""
    fx = fixture(h, w, stride)
    n = 6 if h == 37 else 10
    want = rr.solve(*pr.args_of(fx), fx["T0"], DELTA, stride=stride, numiters=n)
    plain = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride, numiters=n)
    assert not np.array_equal(want[0], plain[0]) and want[1][-1, 0] > 20
    t, n_dev = geo(fx)
    kw = dict(n_dev=n_dev, stride=stride, numiters=n, return_trace=True)
    got = ops.projective_icp(*t, dev(fx["T0"]), huber_delta=DELTA, **kw)
    same_solve(got, want, "%dx%d stride %d" % (h, w, stride))
    taped = ops.projective_icp(*t, dev(fx["T0"]), huber_delta=DELTA, differentiable=True, **kw)
    same_solve(taped, want, "taped")
    # delta = 0 through the new keyword: the call without it
    zero = ops.projective_icp(*t, dev(fx["T0"]), huber_delta=0.0, **kw)
    none = ops.projective_icp(*t, dev(fx["T0"]), **kw)
    same_solve(zero, plain, "delta 0")
    same_solve(none, plain, "no keyword")
    assert np.isfinite(host(got[0])).all()


@pytest.mark.parametrize("h,w,stride", SIZES)
def test_rows_bit_for_bit(ops, h, w, stride):
    fx = fixture(h, w, stride)
    want = rr.rows(*pr.args_of(fx), fx["T"], DELTA, stride=stride)
    used = want.code == 0
    assert (want.weight[used] < 1).sum() >= 10 and (want.weight[used] == 1).sum() >= 10 and (~used).sum() > 5
    if h == 37:
        assert set(np.unique(want.code)) == {0, 1, 2, 3, 4, 5}
    t, n_dev = geo(fx)
    got, weight = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride, huber_delta=DELTA,
                                          return_weights=True)
    torch.cuda.synchronize()
    assert np.array_equal(host(got.code), want.code) and np.array_equal(host(got.row), want.row)
    for name in ("a", "b", "sums"):
        assert np.array_equal(bits(host(getattr(got, name))), bits(getattr(want, name))), name
    assert np.array_equal(bits(host(weight)), bits(want.weight))
    assert int(got.count) == want.count
    # the default return type stays; delta = 0 with the table: 1 for every used slot, the plain sums
    only = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride, huber_delta=DELTA)
    assert isinstance(only, ops.ProjectiveRows) and np.array_equal(bits(host(only.sums)), bits(want.sums))
    plain = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride)
    off, w0 = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride, return_weights=True)
    assert np.array_equal(bits(host(off.sums)), bits(host(plain.sums)))
    assert np.array_equal(host(w0), used.astype(np.float32))


def test_batch_of_nine_crosses_the_launch_boundary(ops):
    """37 x 53, B = 9: 8 sequences per launch, the ninth goes through launches of its own; three different fixtures, one
    behind a device count"""
    a, b = fixture(37, 53, 3), dict(pr.convergence_fixture(37, 53, 3, "facets"))
    c = rr.moved_block(pr.convergence_fixture(37, 53), (slice(9, 24), slice(12, 32)))
    seqs = [a, b, c]
    kw = dict(stride=2, numiters=4)
    want = [rr.solve(*pr.args_of(q), q["T0"], DELTA, **kw) for q in seqs]
    st = lambda k: torch.stack([dev(seqs[i % 3][k]) for i in range(9)])   # noqa: E731
    maps = []
    for i in range(9):
        t, n_dev = geo(seqs[i % 3])
        maps.append((t[6], t[7], None, n_dev))
    T, trace = ops.projective_icp_batch(st("vertex"), st("normal"), st("depth"), st("K"), st("index"), st("model_pose"),
                                        maps, st("T0"), return_trace=True, huber_delta=DELTA, **kw)
    for i in range(9):
        same_solve((T[i], trace[i]), want[i % 3], "sequence %d" % i)
    assert len({want[b][0].tobytes() for b in range(3)}) == 3


# ------------------------------------------------------------------------------------------ 2. the colour solve
THRESHOLDS = [(DELTA, 0.0), (0.0, COLOR_DELTA), (DELTA, COLOR_DELTA)]


@pytest.mark.parametrize("delta,cdelta", THRESHOLDS)
@pytest.mark.parametrize("h,w,stride", [(37, 53, 1), (37, 53, 3), (60, 80, 1), (60, 80, 4)])
def test_colour_solve_and_rows_bit_for_bit(ops, h, w, stride, delta, cdelta):
    fx = color_fixture(h, w, stride)
    n = 6 if h == 37 else 8
    args = pcr.args_of(fx)
    want = rr.color_solve(*args, fx["T0"], WEIGHT, delta, cdelta, stride=stride, numiters=n)
    plain = pcr.solve(*args, fx["T0"], WEIGHT, stride=stride, numiters=n)
    assert not np.array_equal(want[0], plain[0])
    t, n_dev = geo(fx)
    c = [dev(fx["color"]), dev(fx["model"])]
    kw = dict(color_weight=WEIGHT, n_dev=n_dev, stride=stride)
    got = ops.projective_icp_color(*t, dev(fx["T0"]), *c, numiters=n, return_trace=True, huber_delta=delta,
                                   color_huber_delta=cdelta, **kw)
    same_solve(got, want, "%dx%d stride %d" % (h, w, stride))
    zero = ops.projective_icp_color(*t, dev(fx["T0"]), *c, numiters=n, return_trace=True, huber_delta=0.0,
                                    color_huber_delta=0.0, **kw)
    same_solve(zero, plain, "delta 0")
    # one linearisation, with both weight tables
    r = rr.color_rows(*args, fx["T"], WEIGHT, delta, cdelta, stride=stride)
    used = r.code == 0
    if delta > 0:
        assert (r.weight[used] < 1).sum() >= 10 and (r.weight[used] == 1).sum() >= 10
    if cdelta > 0:
        assert (r.color_weight[r.colored] < 1).sum() >= 5 and (r.color_weight[r.colored] == 1).sum() >= 5
    rows_, weight, cweight = ops.projective_icp_color_rows(*t, dev(fx["T"]), *c, huber_delta=delta,
                                                           color_huber_delta=cdelta, return_weights=True, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(host(rows_.code), r.code) and np.array_equal(host(rows_.row), r.row)
    assert np.array_equal(host(rows_.colored) == 1, r.colored)
    for name in ("a", "b", "ac", "bc", "sums"):
        assert np.array_equal(bits(host(getattr(rows_, name))), bits(getattr(r, name))), name
    assert np.array_equal(bits(host(weight)), bits(r.weight))
    assert np.array_equal(bits(host(cweight)), bits(r.color_weight))
    assert int(rows_.count) == r.count and int(rows_.color_count) == r.color_count
    only = ops.projective_icp_color_rows(*t, dev(fx["T"]), *c, huber_delta=delta, color_huber_delta=cdelta, **kw)
    assert isinstance(only, ops.ProjectiveColorRows) and np.array_equal(bits(host(only.sums)), bits(r.sums))


# ------------------------------------------------------------------------------------------ 3. backward
def leaves(fx, count=None, grad=(True, True, True, True)):
    t = {k: dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals", "T0")}
    for k, g in zip(("vertex", "points", "normals", "T0"), grad):
        t[k].requires_grad_(g)
    t["n_dev"] = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    return t


def solve(ops, t, **kw):
    return ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                              t["normals"], t["T0"], n_dev=t["n_dev"], return_trace=True, **kw)


def run(ops, c, grad=(True, True, True, True), T_bar=None):
    """differentiable robust solve of a case and its backward: (pose, trace, [vertex_bar, points_bar, normals_bar,
    T0_bar])"""
    t = leaves(c.fx, c.device_count, grad)
    T, trace = solve(ops, t, stride=c.stride, numiters=c.numiters, differentiable=True, huber_delta=c.delta, **c.kw)
    assert T.grad_fn is not None and not trace.requires_grad
    T.backward(dev(c.T_bar if T_bar is None else T_bar))
    torch.cuda.synchronize()
    return T, trace, [None if t[k].grad is None else host(t[k].grad) for k in ("vertex", "points", "normals", "T0")]


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_kernel_against_the_float64_adjoint(ops, name):
    c = rc.build(name)
    T, trace, got = run(ops, c)
    assert np.array_equal(bits(host(T)), bits(c.assoc.pose)), "the taped forward left the restated solve"
    assert np.array_equal(bits(host(trace)), bits(c.assoc.trace))
    want = rc.reference(c)
    assert (want[3][3] == 0).all() and (got[3][3] == 0).all()
    for out, g, w, gap in zip(rc.OUTPUTS, got, want, rc.GAP[name]):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, out)
        print("%s %s: rel_err %.3g, bound %.3g (gap %.2g)" % (name, out, bc.rel_err(g, w), bc.kernel_bound(gap), gap))
    for out, g, w, gap in zip(rc.OUTPUTS, got, want, rc.GAP[name]):
        assert bc.rel_err(g, w) <= bc.kernel_bound(gap), (name, out, bc.rel_err(g, w), bc.kernel_bound(gap))
    if c.stride > 1:     # pixels off the lattice get exactly zero
        off = np.ones(got[0].shape[:2], bool)
        off[::c.stride, ::c.stride] = False
        assert (got[0][off] == 0).all()
    if c.device_count is not None:   # rows at and beyond the device count are never touched
        assert (got[1][c.device_count:] == 0).all() and (got[2][c.device_count:] == 0).all()
    # bitwise reproducible where the contract says so
    _, _, again = run(ops, c)
    assert np.array_equal(bits(got[0]), bits(again[0])) and np.array_equal(bits(got[3]), bits(again[3]))
    for i in (1, 2):
        assert bc.rel_err(got[i], again[i]) <= MAP_BOUND


@pytest.mark.parametrize("name", rc.NO_INLIER)
def test_no_inlier_passes_the_adjoint_through(ops, name):
    c = rc.build(name)
    T_bar = c.T_bar.copy()
    T_bar[1, 2], T_bar[2, 3] = -0.0, -0.0          # (adding the +0.0 sums of a point stage would turn them into +0.0)
    T, trace, got = run(ops, c, T_bar=T_bar)
    assert np.array_equal(bits(host(T)), bits(np.asarray(c.fx["T0"], np.float32))) and (host(trace) == 0).all()
    assert np.array_equal(bits(got[3][:3]), bits(T_bar[:3])) and (got[3][3] == 0).all()
    for g in got[:3]:
        assert g is not None and (g == 0).all()


def test_outputs_not_asked_for_are_skipped(ops):
    from gradslam_amd import _C
    c = rc.build("conv_s4")
    _, _, full = run(ops, c)
    n_map = c.fx["points"].shape[0]
    side = torch.cuda.Stream()       # (a stream of its own: a workspace of its own, nothing grown by earlier tests)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, _, part = run(ops, c, grad=(True, False, False, True))
        ws = _C.Workspace.get(torch.device("cuda"))
        scratch = ws._bufs["picp_bwd0"].numel()
    torch.cuda.synchronize()
    assert part[1] is None and part[2] is None
    assert np.array_equal(bits(part[0]), bits(full[0])) and np.array_equal(bits(part[3]), bits(full[3]))
    assert scratch < n_map * 3 * 8, (scratch, n_map)        # the map detached: nothing of map size
    _, _, only_map = run(ops, c, grad=(False, True, False, False))
    assert only_map[0] is None and only_map[2] is None and only_map[3] is None
    assert bc.rel_err(only_map[1], full[1]) <= MAP_BOUND


def test_autograd_gives_the_gradients_of_the_tensor_level_call(ops):
    c = rc.build("edge_s3")
    _, _, got = run(ops, c)
    t = leaves(c.fx, c.device_count, (False,) * 4)
    b = lambda k: t[k].unsqueeze(0)      # noqa: E731
    maps = [(t["points"], t["normals"], None, t["n_dev"])]
    kw = dict(stride=c.stride, numiters=c.numiters, **c.kw)
    tapes = torch.empty((1, ops.projective_icp_tape_bytes(c.numiters)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(c.stride, c.numiters, c.kw["damp"], c.kw["dist_thresh"],
                                                        c.kw["angle_thresh"]), huber_delta=c.delta)
    T, _ = ops._picp_solve(opt, b("vertex"), b("normal"), b("depth"), b("K"), b("index"), b("model_pose"), maps, b("T0"),
                           tapes=tapes, return_trace=True)
    assert np.array_equal(bits(host(T[0])), bits(c.assoc.pose))
    vb, rows_, ib = ops.projective_icp_backward_batch(b("vertex"), b("normal"), b("depth"), b("K"), b("index"),
                                                      b("model_pose"), maps, tapes, dev(c.T_bar)[None],
                                                      huber_delta=c.delta, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(vb[0])), bits(got[0])) and np.array_equal(bits(host(ib[0])), bits(got[3]))
    assert bc.rel_err(host(rows_[0][0]), got[1]) <= MAP_BOUND and bc.rel_err(host(rows_[0][1]), got[2]) <= MAP_BOUND
    # the plain backward on the robust tape is another function: the threshold reaches the kernel
    pvb, _, _ = ops.projective_icp_backward_batch(b("vertex"), b("normal"), b("depth"), b("K"), b("index"),
                                                  b("model_pose"), maps, tapes, dev(c.T_bar)[None], **kw)
    assert bc.rel_err(host(pvb[0]), got[0]) > 1e-3


# ------------------------------------------------------------------------------------------ 4. provider and drivers
SEEDS = (0, 1)
KW = dict(dsratio=2, numiters=10)


@pytest.fixture(scope="module")
def sequences():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(L, H, W, seed=s) for s in SEEDS]


def textured_frames(gs):
    seqs = [pcr.textured_sequence(6, H, W, s) for s in ("plane", "wave")]
    st = lambda k: torch.from_numpy(np.stack([q[k][:L] if k != "intrinsics" else q[k] for q in seqs])).cuda()   # noqa: E731
    poses = st("poses")
    poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)


def hand_written_loop(gs, ops, which, frames, weight=0.0, **huber):
    """render the map at the previous pose, the robust solve from that pose (the joint one with a weight), update the
    map: the calls a user would make"""
    from gradslam_amd.slam.fusionutils import update_map_aggregate, update_map_fusion
    B = frames.shape[0]
    m = gs.Pointclouds(device="cuda")
    out, prev = [], None
    K = frames.intrinsics[:, 0].contiguous()
    kw = dict(stride=KW["dsratio"], numiters=KW["numiters"], **huber)
    for s in range(L):
        live = frames[:, s]
        if s > 0:
            counts = [tuple(m._count_of(b)) for b in range(B)]
            maps = [(m._buf["points"][b], m._buf["normals"][b], None, None) + counts[b] for b in range(B)]
            fr = live.to_channels_last()
            geo_ = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K)
            if weight > 0:
                view = ops.render_map_batch([(m._buf["points"][b], None, m._buf["colors"][b], None) + counts[b]
                                             for b in range(B)], prev.view(B, 1, 4, 4), K, H, W)
                model = ops.model_intensity(view.color[:, 0], view.index[:, 0])
                pose = ops.projective_icp_color_batch(*geo_, view.index[:, 0], prev, maps, prev, fr.rgb_image[:, 0], model,
                                                      color_weight=weight, **kw)
            else:
                index = ops.render_map_batch(maps, prev.view(B, 1, 4, 4), K, H, W).index[:, 0]
                pose = ops.projective_icp_batch(*geo_, index, prev, maps, prev, **kw)
            live.poses = pose.view(B, 1, 4, 4)
        if which == "PointFusion":
            m = update_map_fusion(m, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180),
                                  FUSION["sigma"], inplace=True)
        else:
            m = update_map_aggregate(m, live, inplace=True)
        prev = live.poses[:, 0].contiguous()
        out.append(prev.clone())
    return m, torch.stack(out, 1)


def make_slam(gs, which, **extra):
    kw = dict(KW, odom="projicp", device="cuda", **extra)
    if which == "PointFusion":
        kw.update(FUSION)
    return getattr(gs.slam, which)(**kw)


def same_run(got, want):
    (m, poses), (wm, wposes) = got, want
    assert np.array_equal(bits(host(poses)), bits(host(wposes))), np.abs(host(poses) - host(wposes)).max()
    for b in range(poses.shape[0]):
        for g, w_ in zip(map_rows(m, b), map_rows(wm, b)):
            assert g.shape == w_.shape and np.array_equal(bits(g), bits(w_)), b


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_equal_the_hand_written_loop(gs, ops, sequences, which):
    want = hand_written_loop(gs, ops, which, frames_of(gs, sequences), huber_delta=DELTA)
    plain = hand_written_loop(gs, ops, which, frames_of(gs, sequences))
    assert not np.array_equal(host(want[1]), host(plain[1]))                  # the threshold reaches the solve
    same_run(make_slam(gs, which, huber_delta=DELTA)(frames_of(gs, sequences)), want)
    # on the autograd tape (inputs that do not require grad): the same bits
    taped = make_slam(gs, which, huber_delta=DELTA, odom_differentiable=True)(frames_of(gs, sequences))
    same_run(taped, want)
    # and step by step, in place
    slam = make_slam(gs, which, huber_delta=DELTA)
    m, prev, out = gs.Pointclouds(device="cuda"), None, []
    frames = frames_of(gs, sequences)
    for s in range(L):
        live = frames[:, s]
        m, p = slam.step(m, live, prev, inplace=True)
        live.poses = p
        prev = live
        out.append(p[:, 0].clone())
    same_run((m, torch.stack(out, 1)), want)


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_with_the_colour_term_equal_the_hand_written_loop(gs, ops, which):
    huber = dict(huber_delta=DELTA, color_huber_delta=COLOR_DELTA)
    want = hand_written_loop(gs, ops, which, textured_frames(gs), weight=1.0, **huber)
    plain = hand_written_loop(gs, ops, which, textured_frames(gs), weight=1.0)
    assert not np.array_equal(host(want[1]), host(plain[1]))
    same_run(make_slam(gs, which, color_weight=1.0, **huber)(textured_frames(gs)), want)


def test_gradients_reach_the_depth_and_a_late_backward_raises(gs, sequences):
    """the provider with a threshold on the autograd tape; a backward after an in-place prune_ raises"""
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from tests.test_hip_picp_backward import two_frame_map
    prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, differentiable=True, huber_delta=DELTA)
    frames, pc_ = two_frame_map(gs, sequences)
    live = frames[:, 2]
    live.depth_image.requires_grad_(True)
    prev = frames.poses[:, 1:2].clone().requires_grad_(True)
    T = prov.localize(pc_, live, prev)
    assert T.grad_fn is not None
    plain = ProjectiveICPOdometryProvider(numiters=5, stride=2, huber_delta=DELTA).localize(pc_, frames[:, 2], prev.detach())
    none = ProjectiveICPOdometryProvider(numiters=5, stride=2).localize(pc_, frames[:, 2], prev.detach())
    assert np.array_equal(bits(host(T)), bits(host(plain))) and not np.array_equal(host(plain), host(none))
    T[:, 0, :3, 3].sum().backward(retain_graph=True)
    for g in (live.depth_image.grad, prev.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    pc_.prune_(1.5)
    with pytest.raises(RuntimeError, match="changed in place after localize"):
        T.sum().backward()
