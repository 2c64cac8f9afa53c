"""GPU tests of the projective ICP's backward pass (gs_picp_bwd.hip -> gs_projective_icp_backward_batch_f32 ->
ops.ProjectiveICPFunction / projective_icp_backward_batch -> ProjectiveICPOdometryProvider(differentiable=True) ->
ICPSLAM / PointFusion(odom="projicp", odom_differentiable=True)).

The arbiter is the float64 NumPy adjoint (tests/picp_grad_ref.py) at the forward's float32 poses; a kernel output may
differ from it by kernel_bound(gap) of tests/backward_cases.py, the gap being the float32-vs-float64 distance of that
NumPy adjoint on the same case (tests/picp_backward_cases.py; no bound comes from a kernel's output).  vertex_bar and
init_pose_bar have a fixed reduction order and no atomics: runs, batches and skipped outputs are compared for EQUAL
BITS.  points_bar / normals_bar are float64 atomic adds rounded once: compared within the bound."""
import math

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_backward_cases as pc
from tests import picp_ref as pr
from tests.test_hip_picp import FUSION, bits, dev, frames_of, host, three_sequences

pytestmark = pytest.mark.gpu

H, W = 60, 80


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


def leaves(fx, count=None, grad=(True, True, True, True)):
    """the forward's tensors of a fixture; vertex, points, normals, T0 are leaves that require grad where asked"""
    t = {k: dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals", "T0")}
    for k, g in zip(("vertex", "points", "normals", "T0"), grad):
        t[k].requires_grad_(g)
    t["n_dev"] = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    return t


def solve(ops, t, **kw):
    return ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                              t["normals"], t["T0"], n_dev=t["n_dev"], return_trace=True, **kw)


def run(ops, c, grad=(True, True, True, True), T_bar=None):
    """differentiable solve of a case and its backward: (pose, trace, [vertex_bar, points_bar, normals_bar, T0_bar])"""
    t = leaves(c.fx, c.device_count, grad)
    T, trace = solve(ops, t, stride=c.stride, numiters=c.numiters, differentiable=True, **c.kw)
    assert T.grad_fn is not None and not trace.requires_grad
    T.backward(dev(c.T_bar if T_bar is None else T_bar))
    torch.cuda.synchronize()
    return T, trace, [None if t[k].grad is None else host(t[k].grad) for k in ("vertex", "points", "normals", "T0")]


# ------------------------------------------------------------------------------------------ 1. against the float64 adjoint
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_kernel_against_the_float64_adjoint(ops, name):
    """conv_s1 / conv_s4: 19 and 2 chunks, 10 iterations; *_n1: one iteration; edge_s3 / edge_s1: odd sizes, a partial
    last chunk, every reject code, stale index entries and a device count below the bound; stale_dc: 400 stale rows
    behind a device count; radius1: dense collisions in the map scatter."""
    c = pc.build(name)
    T, trace, got = run(ops, c)
    assert np.array_equal(bits(host(T)), bits(c.assoc.pose)), "the taped forward left the restated solve"
    assert np.array_equal(bits(host(trace)), bits(c.assoc.trace))
    want = pc.reference(c)
    assert (want[3][3] == 0).all() and (got[3][3] == 0).all()
    for out, g, w, gap in zip(pc.OUTPUTS, got, want, pc.GAP[name]):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, out)
        err, bound = bc.rel_err(g, w), bc.kernel_bound(gap)
        print("%s %s: rel_err %.3g, bound %.3g (gap %.2g)" % (name, out, err, bound, gap))
    for out, g, w, gap in zip(pc.OUTPUTS, got, want, pc.GAP[name]):
        assert bc.rel_err(g, w) <= bc.kernel_bound(gap), (name, out, bc.rel_err(g, w), bc.kernel_bound(gap))
    if c.stride > 1:     # pixels off the lattice get exactly zero
        off = np.ones(got[0].shape[:2], bool)
        off[::c.stride, ::c.stride] = False
        assert (got[0][off] == 0).all()
    if c.device_count is not None:   # rows at and beyond the device count are never touched
        assert (got[1][c.device_count:] == 0).all() and (got[2][c.device_count:] == 0).all()


# ------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("name", ["conv_s1", "edge_s3", "radius1"])
def test_taped_forward_and_deterministic_outputs_bit_for_bit(ops, name):
    c = pc.build(name)
    t = leaves(c.fx, c.device_count, (False,) * 4)
    kw = dict(stride=c.stride, numiters=c.numiters, **c.kw)
    plain = solve(ops, t, **kw)
    assert not plain[0].requires_grad
    T, trace, a = run(ops, c)
    assert np.array_equal(bits(host(T)), bits(host(plain[0]))) and np.array_equal(bits(host(trace)), bits(host(plain[1])))
    _, _, b = run(ops, c)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[3]), bits(b[3]))
    for i in (1, 2):        # the map scatter: float64 atomics, the same up to the order of the float64 additions
        assert bc.rel_err(a[i], b[i]) <= bc.FLOOR_ULPS * bc.EPS32


# ------------------------------------------------------------------------------------------ 3. no inlier
@pytest.mark.parametrize("name", pc.NO_INLIER)
def test_no_inlier_passes_the_adjoint_through(ops, name):
    c = pc.build(name)
    T_bar = c.T_bar.copy()
    T_bar[1, 2], T_bar[2, 3] = -0.0, -0.0          # (adding the +0.0 sums of a point stage would turn them into +0.0)
    T, trace, got = run(ops, c, T_bar=T_bar)
    assert np.array_equal(bits(host(T)), bits(np.asarray(c.fx["T0"], np.float32))) and (host(trace) == 0).all()
    assert np.array_equal(bits(got[3][:3]), bits(T_bar[:3])) and (got[3][3] == 0).all()
    for g in got[:3]:
        assert g is not None and (g == 0).all()


# ------------------------------------------------------------------------------------------ 4. batches
def batch_run(ops, seqs, T_bars, **kw):
    st = lambda k: torch.stack([dev(q[k]) for q in seqs])   # noqa: E731
    vertex, T0 = st("vertex").requires_grad_(True), st("T0").requires_grad_(True)
    maps = [(dev(q["points"]).requires_grad_(True), dev(q["normals"]).requires_grad_(True), None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in seqs]
    T = ops.projective_icp_batch(vertex, st("normal"), st("depth"), st("K"), st("index"), st("model_pose"), maps, T0,
                                 differentiable=True, **kw)
    T.backward(torch.stack([dev(x) for x in T_bars]))
    torch.cuda.synchronize()
    return host(T), host(vertex.grad), [(host(m[0].grad), host(m[1].grad)) for m in maps], host(T0.grad)


def single_run(ops, q, T_bar, **kw):
    t = leaves(q, q["n_dev"])
    T, _ = solve(ops, t, differentiable=True, **kw)
    T.backward(dev(T_bar))
    torch.cuda.synchronize()
    return host(T), [host(t[k].grad) for k in ("vertex", "points", "normals", "T0")]


MAP_BOUND = bc.kernel_bound(0.0)    # two runs of the same float64 atomic sums, rounded once: float32 ulps of the scale


def test_batch_of_three_equals_three_single_calls(ops):
    seqs = three_sequences()
    kw = dict(stride=2, numiters=5)
    T_bars = [bc.weights((4, 4), 40 + b) for b in range(3)]
    T, vb, mb, ib = batch_run(ops, seqs, T_bars, **kw)
    for b, q in enumerate(seqs):
        sT, (svb, spb, snb, sib) = single_run(ops, q, T_bars[b], **kw)
        assert np.array_equal(bits(T[b]), bits(sT)), b
        assert np.array_equal(bits(vb[b]), bits(svb)) and np.array_equal(bits(ib[b]), bits(sib)), b
        assert np.abs(svb).max() > 0 and np.abs(spb).max() > 0 and np.abs(snb).max() > 0
        assert mb[b][0].shape == spb.shape and bc.rel_err(mb[b][0], spb) <= MAP_BOUND, (b, bc.rel_err(mb[b][0], spb))
        assert bc.rel_err(mb[b][1], snb) <= MAP_BOUND, (b, bc.rel_err(mb[b][1], snb))


def test_batch_of_nine_crosses_the_launch_boundary(ops):
    """8 sequences per launch: the ninth goes through launches of its own"""
    seqs = three_sequences()
    kw = dict(stride=4, numiters=4)
    T_bars = [bc.weights((4, 4), 50 + (i % 3)) for i in range(9)]
    T, vb, mb, ib = batch_run(ops, [seqs[i % 3] for i in range(9)], T_bars, **kw)
    for i in range(3, 9):
        assert np.array_equal(bits(vb[i]), bits(vb[i % 3])) and np.array_equal(bits(ib[i]), bits(ib[i % 3])), i
        assert bc.rel_err(mb[i][0], mb[i % 3][0]) <= MAP_BOUND and bc.rel_err(mb[i][1], mb[i % 3][1]) <= MAP_BOUND, i
    for b in range(3):
        _, (svb, spb, snb, sib) = single_run(ops, seqs[b], T_bars[b], **kw)
        assert np.array_equal(bits(vb[b]), bits(svb)) and np.array_equal(bits(ib[b]), bits(sib)), b
        assert bc.rel_err(mb[b][0], spb) <= MAP_BOUND and bc.rel_err(mb[b][1], snb) <= MAP_BOUND, b


# ------------------------------------------------------------------------------------------ 5. skipped outputs
def test_outputs_not_asked_for_are_skipped(ops):
    from gradslam_amd import _C
    c = pc.build("conv_s4")
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
    # the common case -- a loss reaching the depth and the initial pose, the map detached -- holds nothing of map size
    assert scratch < n_map * 3 * 8, (scratch, n_map)
    _, _, only_map = run(ops, c, grad=(False, True, False, False))
    assert only_map[0] is None and only_map[2] is None and only_map[3] is None
    assert bc.rel_err(only_map[1], full[1]) <= MAP_BOUND


# ------------------------------------------------------------------------------------------ 6. through the provider
SEEDS = (0, 1)
KW = dict(dsratio=2, numiters=10)


@pytest.fixture(scope="module")
def sequences():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(3, H, W, seed=s) for s in SEEDS]


def make_slam(gs, **extra):
    return gs.slam.PointFusion(odom="projicp", device="cuda", **KW, **FUSION, **extra)


def two_frame_map(gs, sequences, grad=False):
    """the map after frames 0 and 1 (ground-truth poses), frame 2 as the live frame, the pose of frame 1"""
    frames = frames_of(gs, sequences, first_pose_only=False)
    if grad:
        frames.depth_image.requires_grad_(True)
    slam = gs.slam.PointFusion(odom="gt", device="cuda", **FUSION)
    pc_ = gs.Pointclouds(device="cuda")
    for s in range(2):
        pc_, _ = slam.step(pc_, frames[:, s], None, inplace=True)
    return frames, pc_


def test_provider_puts_the_pose_on_the_tape_and_guards_a_late_backward(gs, sequences):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, differentiable=True)
    for change in ("prune", "step"):
        frames, pc_ = two_frame_map(gs, sequences)
        live = frames[:, 2]
        live.depth_image.requires_grad_(True)
        prev = frames.poses[:, 1:2].clone().requires_grad_(True)
        T = prov.localize(pc_, live, prev)
        assert tuple(T.shape) == (len(SEEDS), 1, 4, 4) and T.grad_fn is not None
        plain = ProjectiveICPOdometryProvider(numiters=5, stride=2).localize(pc_, frames[:, 2], prev.detach())
        assert not plain.requires_grad and np.array_equal(bits(host(T)), bits(host(plain)))
        if change == "prune":
            pc_.prune_(1.5)
        else:
            again = frames_of(gs, sequences, first_pose_only=False)
            gs.slam.PointFusion(odom="gt", device="cuda", **FUSION).step(pc_, again[:, 2], None, inplace=True)
        with pytest.raises(RuntimeError, match="changed in place after localize"):
            T.sum().backward()
    # without a change in between the backward runs and reaches the depth and the initial pose
    frames, pc_ = two_frame_map(gs, sequences)
    live = frames[:, 2]
    live.depth_image.requires_grad_(True)
    prev = frames.poses[:, 1:2].clone().requires_grad_(True)
    prov.localize(pc_, live, prev)[:, 0, :3, 3].sum().backward()
    for g in (live.depth_image.grad, prev.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0


@pytest.mark.parametrize("inplace", [False, True])
def test_backward_after_a_taped_update_of_a_map_built_in_place(gs, ops, sequences, inplace):
    """a warm-up without grad, then a differentiable window: the map comes from ordinary in-place steps, its counts live
    on the device; the taped update that follows the localisation reads them back, which changes no buffer and must not
    trip the guard of the backward"""
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam.fusionutils import update_map_fusion
    prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, differentiable=True)
    frames, pc_ = two_frame_map(gs, sequences)
    assert not any(t.requires_grad for t in pc_._buf["points"])
    if ops.DEVICE_COUNTS:
        assert pc_._dcount, "the in-place steps left the counts on the device"
    live = frames[:, 2]
    live.depth_image.requires_grad_(True)
    prev = frames.poses[:, 1:2].clone().requires_grad_(True)
    T = prov.localize(pc_, live, prev)
    live.poses = T
    rewrites = pc_._rewrites()
    out = update_map_fusion(pc_, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180), FUSION["sigma"],
                            inplace=inplace)
    assert (out is pc_) == inplace and not pc_._dcount and pc_._rewrites() == rewrites
    assert all(t.requires_grad for t in out._buf["points"])
    (T[:, 0, :3, 3].sum() + sum(t.sum() for t in out._buf["points"])).backward()
    torch.cuda.synchronize()
    for g in (live.depth_image.grad, prev.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0


def test_backward_after_a_taped_map_update_equals_the_ops_level_call(gs, ops, sequences):
    """the map update that follows ran on the tape: it gave the map new tensors and left the saved ones intact"""
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam.fusionutils import update_map_fusion
    prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, differentiable=True)
    frames, pc_ = two_frame_map(gs, sequences, grad=True)     # (depth requires grad: the map itself is on the tape)
    B = len(SEEDS)
    assert all(t.requires_grad for t in pc_._buf["points"])
    live = frames[:, 2]
    prev = frames.poses[:, 1:2].clone().requires_grad_(True)
    fr = live.to_channels_last()
    vertex = fr.vertex_map
    K = fr.intrinsics[:, 0].contiguous().float()
    P, N = list(pc_._buf["points"]), list(pc_._buf["normals"])
    maps = [(P[b], N[b], None, None) + tuple(pc_._count_of(b)) for b in range(B)]
    T = prov.localize(pc_, live, prev)
    # the ops-level call on the same inputs, before the map moves on
    p0 = prev.reshape(B, 4, 4)
    index = ops.render_map_batch([(m[0].detach(), None) + m[2:] for m in maps], p0.detach().view(B, 1, 4, 4), K, H, W).index
    T2 = ops.projective_icp_batch(vertex[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, index[:, 0],
                                  p0.detach(), maps, p0, stride=2, numiters=5, differentiable=True)
    assert np.array_equal(bits(host(T[:, 0])), bits(host(T2)))
    Tb = torch.stack([dev(bc.weights((4, 4), 60 + b)) for b in range(B)])
    want = torch.autograd.grad(T2, [vertex, prev] + P + N, Tb, retain_graph=True)
    live.poses = T.detach()
    generation = pc_._generation
    out = update_map_fusion(pc_, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180), FUSION["sigma"],
                            inplace=True)
    assert out is pc_ and pc_._generation > generation and pc_._buf["points"][0] is not P[0]
    got = torch.autograd.grad(T[:, 0], [vertex, prev] + P + N, Tb)
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = host(g), host(w)
        assert np.abs(w).max() > 0, i
        if i < 2:
            assert np.array_equal(bits(g), bits(w)), i
        else:
            assert bc.rel_err(g, w) <= MAP_BOUND, (i, bc.rel_err(g, w))


# ------------------------------------------------------------------------------------------ 7. through the drivers
def hand_written_chain(gs, ops, frames):
    """the frame loop of PointFusion(odom="projicp", odom_differentiable=True) out of the ops-level Functions: the taped
    map update, the plain render of the index image, ProjectiveICPFunction"""
    from gradslam_amd.slam.fusionutils import update_map_fusion
    B, L = frames.shape[:2]
    pc_ = gs.Pointclouds(device="cuda")
    prev, out = None, []
    for s in range(L):
        live = frames[:, s]
        if s > 0:
            fr = live.to_channels_last()
            fr._sigma_hint = float(FUSION["sigma"])
            K = fr.intrinsics[:, 0].contiguous().float()
            maps = [(pc_._buf["points"][b], pc_._buf["normals"][b], None, None) + tuple(pc_._count_of(b)) for b in range(B)]
            index = ops.render_map_batch([(m[0].detach(), None) + m[2:] for m in maps], prev.detach().view(B, 1, 4, 4), K,
                                         H, W).index[:, 0]
            T = ops.projective_icp_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, index,
                                         prev.detach(), maps, prev, stride=KW["dsratio"], numiters=KW["numiters"],
                                         differentiable=True)
            live.poses = T.unsqueeze(1)
        pc_ = update_map_fusion(pc_, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180),
                                FUSION["sigma"], inplace=True)
        prev = live.poses[:, 0].contiguous()
        out.append(prev)
    return torch.stack(out, 1)


@pytest.mark.parametrize("how", ["forward", "step_out_of_place"])
def test_drivers_carry_the_gradient_to_earlier_frames(gs, ops, sequences, how):
    """three 60 x 80 frames: a loss on the last pose reaches the depth of all three frames -- of frame 2 through its own
    vertex map (bitwise reproducible), of frames 0 and 1 through the map rows they wrote (the float64 atomics of the map
    scatter, rounded once, then the linear backward of the map update: MAP_BOUND of the largest element)"""
    B = len(SEEDS)
    Tb = torch.stack([dev(bc.weights((4, 4), 70 + b)) for b in range(B)])

    def loss_grad(poses, depth):
        assert poses.grad_fn is not None
        (g,) = torch.autograd.grad(poses[:, -1], depth, Tb)
        torch.cuda.synchronize()
        return host(g)

    frames = frames_of(gs, sequences)
    frames.depth_image.requires_grad_(True)
    slam = make_slam(gs, odom_differentiable=True)
    if how == "forward":
        _, poses = slam(frames)
    else:
        pc_, prev, out = gs.Pointclouds(device="cuda"), None, []
        for s in range(3):
            live = frames[:, s]
            pc_, p = slam.step(pc_, live, prev, inplace=False)
            live.poses = p
            prev = live
            out.append(p[:, 0])
        poses = torch.stack(out, 1)
    got = loss_grad(poses, frames.depth_image)
    ref_frames = frames_of(gs, sequences)
    ref_frames.depth_image.requires_grad_(True)
    ref_poses = hand_written_chain(gs, ops, ref_frames)
    want = loss_grad(ref_poses, ref_frames.depth_image)
    assert np.array_equal(bits(host(poses)), bits(host(ref_poses)))
    assert np.isfinite(got).all()
    for s in range(3):
        assert np.abs(got[:, s]).max() > 0, s
        print("%s frame %d: |depth_bar| max %.3g, rel_err to the hand-written chain %.3g" % (
            how, s, np.abs(got[:, s]).max(), bc.rel_err(got[:, s], want[:, s])))
    assert np.array_equal(bits(got[:, 2]), bits(want[:, 2]))
    for s in range(2):
        assert bc.rel_err(got[:, s], want[:, s]) <= MAP_BOUND, (s, bc.rel_err(got[:, s], want[:, s]))


def test_switch_off_keeps_the_bits_and_the_detachment(gs, sequences):
    """without the switch the drivers return what they returned before it existed: detached poses (and the warning of a
    requires-grad input); with it, on inputs that do not require grad, the taped solve returns the same bits"""
    _, off = make_slam(gs)(frames_of(gs, sequences))
    _, on = make_slam(gs, odom_differentiable=True)(frames_of(gs, sequences))
    assert off.grad_fn is None and not off.requires_grad and on.grad_fn is None
    assert np.array_equal(bits(host(off)), bits(host(on)))
    assert not np.array_equal(host(off[:, 1]), host(off[:, 0]))
    frames = frames_of(gs, sequences)
    frames.depth_image.requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        _, poses = make_slam(gs)(frames)
    assert poses.grad_fn is None and np.array_equal(bits(host(poses)), bits(host(off)))
