"""GPU tests of the projective ICP's Huber threshold from the residuals' median (gs_picp_scale.hip in front of the robust
kernels: the *_scaled_* entry points -> ops.projective_icp*(huber_k=...) -> ProjectiveICPOdometryProvider -> ICPSLAM /
PointFusion(odom="projicp", huber_k=...)).

Forward: the selection is exact (integer counting over the bit patterns of |b|), every other operation is restated in the
same order by tests/picp_scale_ref.py, so every comparison -- thresholds, weights, sums, poses, traces -- is for EQUAL
BITS.  Backward: the arbiter is the float64 NumPy adjoint of the same file at the forward's float32 poses and thresholds;
a kernel output may differ from it by kernel_bound(gap) of tests/backward_cases.py, the gap being the float32-vs-float64
distance of that NumPy adjoint (tests/picp_scale_backward_cases.py; no bound comes from a kernel's output)."""
import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_color_ref as pcr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_backward_cases as sc
from tests import picp_scale_ref as sr
from tests.test_hip_picp import bits, dev, edge_fixture, frames_of, host
from tests.test_hip_picp_color import color_edge_fixture
from tests.test_hip_picp_robust import (MAP_BOUND, geo, hand_written_loop, leaves, make_slam, same_run, same_solve, solve,
                                        textured_frames)

pytestmark = pytest.mark.gpu

F = np.float32
K = sr.K_HUBER
H, W, L = 60, 80, 4
WEIGHT, COLOR_DELTA = 0.2, 0.02


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


def same_scaled(got, want, what=""):
    """(pose, trace, thresholds) of the device against the restatement, bit for bit"""
    same_solve(got[:2], want[:2], what)
    assert np.array_equal(bits(host(got[2])), bits(want[2])), (what, host(got[2]), want[2])


# ------------------------------------------------------------------------------------------ 1. the selection alone
def plane_fixture(h, w, e, used):
    """A scene in which the residual of pixel i is e[i] EXACTLY: identity live and model poses, a fronto-parallel plane at
    z = 1 whose vertices are the unprojected pixel centres (focal length 64 and an integer principal point: a pixel
    projects onto itself without rounding), live and map normals (0, 0, 1), map row i = vertex i displaced by e[i] along
    z.  e: multiples of 2^-23 below the 0.1 m gate, so that 1 + e and (1 + e) - 1 are exact.  used (h * w) bool: the
    depth elsewhere is 0."""
    f, cx, cy = 64.0, float(w // 2), float(h // 2)
    Kc = np.eye(4, dtype=F)
    Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2] = f, f, cx, cy
    hh, ww = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    vertex = np.stack([(ww - F(cx)) / F(f), (hh - F(cy)) / F(f), np.ones((h, w), F)], -1).astype(F)
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    depth = np.where(used.reshape(h, w), F(1.0), F(0.0)).astype(F)
    points = vertex.reshape(-1, 3).copy()
    points[:, 2] += np.asarray(e, F)
    normals = normal.reshape(-1, 3).copy()
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    eye = np.eye(4, dtype=F)
    return dict(vertex=vertex, normal=normal, depth=depth, K=Kc, index=index, model_pose=eye, points=points,
                normals=normals, count=h * w, T=eye, T0=eye)


U = F(2.0 ** -23)


def _multiset(name, n, rng):
    if name == "all equal":
        return np.full(n, 2.0 ** -8, F)
    if name == "half and half":                      # an even count: the lower median is the smaller value
        return np.where(np.arange(n) % 2 == 0, F(2.0 ** -7), F(2.0 ** -9)).astype(F)
    if name == "mixed signs":
        return np.where(rng.integers(0, 2, n) == 0, F(2.0 ** -6), F(-2.0 ** -6)).astype(F)
    if name == "low bits only":                      # one bin in the first two passes: the last pass decides
        e = (F(2.0 ** -4) + rng.integers(0, 64, n).astype(F) * U).astype(F)
        assert np.unique(e.view(np.uint32) >> 10).size == 1
        return e
    if name == "top bits only":                      # the first pass decides
        return np.array([2.0 ** -20, 2.0 ** -16, 2.0 ** -12, 2.0 ** -8, 2.0 ** -5], F)[rng.integers(0, 5, n)]
    if name == "mostly zeros":                       # median 0: threshold 0, every weight 1, the plain sums
        return np.where(np.arange(n) % 5 < 3, F(0.0), F(2.0 ** -7)).astype(F)
    if name == "random":
        return (rng.integers(-700000, 700000, n).astype(F) * U).astype(F)
    raise KeyError(name)


MULTISETS = ["all equal", "half and half", "mixed signs", "low bits only", "top bits only", "mostly zeros", "random"]
# (h, w, used count or None = every pixel): 1, 2 and the counts around the 256-slot chunk; 513 crosses two boundaries
COUNTS = [(16, 17, 1), (16, 17, 2), (16, 17, 255), (16, 17, 256), (16, 17, 257), (16, 17, None), (37, 53, 513),
          (37, 53, None)]


@pytest.mark.parametrize("name", MULTISETS)
def test_selection_alone_through_the_rows_entry(ops, name):
    rng = np.random.default_rng(11)
    for h, w, n in COUNTS:
        used = np.zeros(h * w, bool)
        used[rng.permutation(h * w)[: h * w if n is None else n]] = True
        e = _multiset(name, h * w, rng)
        fx = plane_fixture(h, w, e, used)
        want = sr.rows(*pr.args_of(fx), fx["T"], K)
        # the residuals are exactly the chosen ones
        assert np.array_equal(want.code == 0, used) and np.array_equal(bits(want.b[used]), bits(e[used])), (name, h, w, n)
        med = np.sort(np.abs(e[used]))[(used.sum() - 1) // 2]
        assert bits(want.delta) == bits(sr.constant(K) * med)
        t, _ = geo(fx)
        got, weight, delta = ops.projective_icp_rows(*t, dev(fx["T"]), huber_k=K, return_weights=True)
        torch.cuda.synchronize()
        what = (name, h, w, n)
        assert bits(host(delta)[0]) == bits(want.delta), (what, host(delta), want.delta)
        assert np.array_equal(bits(host(weight)), bits(want.weight)), what
        assert np.array_equal(bits(host(got.sums)), bits(want.sums)), what
        assert np.array_equal(bits(host(got.b)), bits(want.b)) and int(got.count) == want.count == used.sum(), what
        if name == "mostly zeros" and (n is None or n > 2):
            plain = ops.projective_icp_rows(*t, dev(fx["T"]))
            assert bits(want.delta) == bits(F(0.0)) and np.array_equal(host(weight), used.astype(F))
            assert np.array_equal(bits(host(got.sums)), bits(host(plain.sums))), what
        # a floor above the product takes its place
        _, _, floored = ops.projective_icp_rows(*t, dev(fx["T"]), huber_k=K, huber_delta=0.5, return_weights=True)
        assert bits(host(floored)[0]) == bits(F(0.5)), what


def test_no_used_slot_reports_a_zero_threshold(ops):
    fx = plane_fixture(16, 17, np.full(272, 2.0 ** -8, F), np.zeros(272, bool))
    t, _ = geo(fx)
    got, weight, delta = ops.projective_icp_rows(*t, dev(fx["T"]), huber_k=K, huber_delta=0.01, return_weights=True)
    assert bits(host(delta)[0]) == bits(F(0.0)) and int(got.count) == 0 and (host(weight) == 0).all()


# ------------------------------------------------------------------------------------------ 2. rows and solve
def fixture(h, w, stride):
    """37 x 53: the edge fixture (every reject code, stale entries, a device count), linearised 4 cm off; else the
    convergence fixture, 60 x 80 with the moved block"""
    if (h, w) == (37, 53):
        return dict(edge_fixture(h, w, stride))
    fx = pr.convergence_fixture(h, w)
    fx = rr.moved_block(fx) if (h, w) == (60, 80) else dict(fx)
    fx["T"] = fx["T0"]
    return fx


SIZES = [(37, 53, 3), (37, 53, 1), (60, 80, 1), (60, 80, 4), (257, 257, 1)]   # (257 x 257: 259 chunks, two finish tiles)


@pytest.mark.parametrize("h,w,stride", SIZES)
def test_rows_bit_for_bit(ops, h, w, stride):
    fx = fixture(h, w, stride)
    want = sr.rows(*pr.args_of(fx), fx["T"], K, stride=stride)
    used = want.code == 0
    assert (want.weight[used] < 1).sum() >= 10 and (want.weight[used] == 1).sum() >= 10 and (~used).sum() > 5
    if h == 37:
        assert set(np.unique(want.code)) == {0, 1, 2, 3, 4, 5}
    t, n_dev = geo(fx)
    got, weight, delta = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride, huber_k=K,
                                                 return_weights=True)
    torch.cuda.synchronize()
    assert bits(host(delta)[0]) == bits(want.delta), (host(delta), want.delta)
    assert np.array_equal(host(got.code), want.code) and np.array_equal(host(got.row), want.row)
    for name in ("a", "b", "sums"):
        assert np.array_equal(bits(host(getattr(got, name))), bits(getattr(want, name))), name
    assert np.array_equal(bits(host(weight)), bits(want.weight)) and int(got.count) == want.count
    only = ops.projective_icp_rows(*t, dev(fx["T"]), n_dev=n_dev, stride=stride, huber_k=K)
    assert isinstance(only, ops.ProjectiveRows) and np.array_equal(bits(host(only.sums)), bits(want.sums))


@pytest.mark.parametrize("h,w,stride", SIZES)
def test_solve_bit_for_bit(ops, h, w, stride):
    """pose, trace and thresholds; the taped forward; huber_k = 0 and the absent keyword; a floor above every threshold"""
    fx = fixture(h, w, stride)
    n = {37: 6, 60: 10, 257: 3}[h]
    kwr = dict(stride=stride, numiters=n)
    want = sr.solve(*pr.args_of(fx), fx["T0"], K, **kwr)
    plain = pr.solve(*pr.args_of(fx), fx["T0"], **kwr)
    assert not np.array_equal(want[0], plain[0]) and want[1][-1, 0] > 20 and np.unique(want[2]).size > 1
    t, n_dev = geo(fx)
    kw = dict(n_dev=n_dev, return_trace=True, **kwr)
    got = ops.projective_icp(*t, dev(fx["T0"]), huber_k=K, return_scale=True, **kw)
    same_scaled(got, want, "%dx%d stride %d" % (h, w, stride))
    same_solve(ops.projective_icp(*t, dev(fx["T0"]), huber_k=K, **kw), want[:2], "without the thresholds")
    taped = ops.projective_icp(*t, dev(fx["T0"]), huber_k=K, return_scale=True, differentiable=True, **kw)
    same_scaled(taped, want, "taped")
    same_solve(ops.projective_icp(*t, dev(fx["T0"]), huber_k=0.0, **kw), plain, "huber_k 0")
    same_solve(ops.projective_icp(*t, dev(fx["T0"]), **kw), plain, "no keyword")
    floor = 0.25
    assert floor > want[2].max()
    const = rr.solve(*pr.args_of(fx), fx["T0"], floor, **kwr)
    high = ops.projective_icp(*t, dev(fx["T0"]), huber_k=K, huber_delta=floor, return_scale=True, **kw)
    same_solve(high[:2], const, "a floor above every threshold")
    assert (host(high[2]) == F(floor)).all()
    off = ops.projective_icp(*t, dev(fx["T0"]), huber_delta=0.005, return_scale=True, **kw)   # huber_k 0: the constant
    assert (host(off[2]) == F(0.005)).all() and off[2].shape == (n,)


def test_batch_of_nine_crosses_the_launch_boundary(ops):
    """37 x 53, B = 9: 8 sequences per launch, the ninth goes through launches of its own; three different scenes, one
    behind a device count: every sequence has its own thresholds and equals its lone solve"""
    a, b = dict(edge_fixture(37, 53, 3)), dict(pr.convergence_fixture(37, 53, 3, "facets"))
    c = rr.moved_block(pr.convergence_fixture(37, 53), (slice(9, 24), slice(12, 32)))
    seqs = [a, b, c]
    kw = dict(stride=2, numiters=4)
    want = [sr.solve(*pr.args_of(q), q["T0"], K, **kw) for q in seqs]
    assert len({w_[2].tobytes() for w_ in want}) == 3
    st = lambda k: torch.stack([dev(seqs[i % 3][k]) for i in range(9)])   # noqa: E731
    maps = []
    for i in range(9):
        t, n_dev = geo(seqs[i % 3])
        maps.append((t[6], t[7], None, n_dev))
    T, trace, scale = ops.projective_icp_batch(st("vertex"), st("normal"), st("depth"), st("K"), st("index"),
                                               st("model_pose"), maps, st("T0"), return_trace=True, return_scale=True,
                                               huber_k=K, **kw)
    assert scale.shape == (9, 4)
    for i in range(9):
        same_scaled((T[i], trace[i], scale[i]), want[i % 3], "sequence %d" % i)
        t, n_dev = geo(seqs[i % 3])
        lone = ops.projective_icp(*t, dev(seqs[i % 3]["T0"]), n_dev=n_dev, huber_k=K, return_trace=True, return_scale=True,
                                  **kw)
        for g, l_ in zip((T[i], trace[i], scale[i]), lone):
            assert np.array_equal(bits(host(g)), bits(host(l_))), i


# ------------------------------------------------------------------------------------------ 3. the joint solve
@pytest.mark.parametrize("cdelta", [0.0, COLOR_DELTA])
@pytest.mark.parametrize("h,w,stride", [(37, 53, 3), (60, 80, 1), (60, 80, 4)])
def test_colour_solve_bit_for_bit(ops, h, w, stride, cdelta):
    if (h, w) == (37, 53):
        fx = dict(color_edge_fixture(h, w, stride))
    else:
        fx = rr.moved_block(pcr.textured_fixture(h, w, scene="plane"))
    n = 6 if h == 37 else 8
    args = pcr.args_of(fx)
    want = sr.color_solve(*args, fx["T0"], WEIGHT, K, 0.0, cdelta, stride=stride, numiters=n)
    const = rr.color_solve(*args, fx["T0"], WEIGHT, 0.005, cdelta, stride=stride, numiters=n)
    assert not np.array_equal(want[0], const[0]) and np.unique(want[2]).size > 1
    t, n_dev = geo(fx)
    c = [dev(fx["color"]), dev(fx["model"])]
    kw = dict(color_weight=WEIGHT, n_dev=n_dev, stride=stride, numiters=n, return_trace=True, color_huber_delta=cdelta)
    got = ops.projective_icp_color(*t, dev(fx["T0"]), *c, huber_k=K, return_scale=True, **kw)
    same_scaled(got, want, "%dx%d stride %d colour delta %g" % (h, w, stride, cdelta))
    # huber_k = 0 is the call without the keyword
    zero = ops.projective_icp_color(*t, dev(fx["T0"]), *c, huber_k=0.0, huber_delta=0.005, **kw)
    same_solve(zero, const, "huber_k 0")


# ------------------------------------------------------------------------------------------ 4. backward
def run(ops, c, grad=(True, True, True, True), T_bar=None):
    """differentiable scaled solve of a case and its backward: (pose, trace, thresholds, [vertex_bar, points_bar,
    normals_bar, T0_bar])"""
    t = leaves(c.fx, c.device_count, grad)
    T, trace, scale = solve(ops, t, stride=c.stride, numiters=c.numiters, differentiable=True, huber_k=c.huber_k,
                            return_scale=True, **c.kw)
    assert T.grad_fn is not None and not trace.requires_grad and not scale.requires_grad
    T.backward(dev(c.T_bar if T_bar is None else T_bar))
    torch.cuda.synchronize()
    return T, trace, scale, [None if t[k].grad is None else host(t[k].grad) for k in ("vertex", "points", "normals", "T0")]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_kernel_against_the_float64_adjoint(ops, name):
    c = sc.build(name)
    T, trace, scale, got = run(ops, c)
    assert np.array_equal(bits(host(T)), bits(c.assoc.pose)), "the taped forward left the restated solve"
    assert np.array_equal(bits(host(trace)), bits(c.assoc.trace))
    assert np.array_equal(bits(host(scale)), bits(c.assoc.deltas))
    want = sc.reference(c)
    assert (want[3][3] == 0).all() and (got[3][3] == 0).all()
    for out, g, w, gap in zip(sc.OUTPUTS, got, want, sc.GAP[name]):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, out)
        print("%s %s: rel_err %.3g, bound %.3g (gap %.2g)" % (name, out, bc.rel_err(g, w), bc.kernel_bound(gap), gap))
    for out, g, w, gap in zip(sc.OUTPUTS, got, want, sc.GAP[name]):
        assert bc.rel_err(g, w) <= bc.kernel_bound(gap), (name, out, bc.rel_err(g, w), bc.kernel_bound(gap))
    if c.stride > 1:     # pixels off the lattice get exactly zero
        off = np.ones(got[0].shape[:2], bool)
        off[::c.stride, ::c.stride] = False
        assert (got[0][off] == 0).all()
    if c.device_count is not None:   # rows at and beyond the device count are never touched
        assert (got[1][c.device_count:] == 0).all() and (got[2][c.device_count:] == 0).all()
    # bitwise reproducible where the contract says so
    _, _, _, again = run(ops, c)
    assert np.array_equal(bits(got[0]), bits(again[0])) and np.array_equal(bits(got[3]), bits(again[3]))
    for i in (1, 2):
        assert bc.rel_err(got[i], again[i]) <= MAP_BOUND


@pytest.mark.parametrize("name", sc.NO_INLIER)
def test_no_inlier_passes_the_adjoint_through(ops, name):
    c = sc.build(name)
    T_bar = c.T_bar.copy()
    T_bar[1, 2], T_bar[2, 3] = -0.0, -0.0          # (adding the +0.0 sums of a point stage would turn them into +0.0)
    T, trace, scale, got = run(ops, c, T_bar=T_bar)
    assert np.array_equal(bits(host(T)), bits(np.asarray(c.fx["T0"], F))) and (host(trace) == 0).all()
    assert np.array_equal(bits(host(scale)), bits(np.zeros(c.numiters, F)))
    assert np.array_equal(bits(got[3][:3]), bits(T_bar[:3])) and (got[3][3] == 0).all()
    for g in got[:3]:
        assert g is not None and (g == 0).all()


def test_outputs_not_asked_for_are_skipped(ops):
    c = sc.build("conv_s4")
    _, _, _, full = run(ops, c)
    _, _, _, part = run(ops, c, grad=(True, False, False, True))
    assert part[1] is None and part[2] is None
    assert np.array_equal(bits(part[0]), bits(full[0])) and np.array_equal(bits(part[3]), bits(full[3]))
    _, _, _, only_map = run(ops, c, grad=(False, True, False, False))
    assert only_map[0] is None and only_map[2] is None and only_map[3] is None
    assert bc.rel_err(only_map[1], full[1]) <= MAP_BOUND


def test_autograd_gives_the_gradients_of_the_tensor_level_call(ops):
    c = sc.build("edge_s3")
    _, _, _, got = run(ops, c)
    t = leaves(c.fx, c.device_count, (False,) * 4)
    b = lambda k: t[k].unsqueeze(0)      # noqa: E731
    maps = [(t["points"], t["normals"], None, t["n_dev"])]
    kw = dict(stride=c.stride, numiters=c.numiters, **c.kw)
    tapes = torch.empty((1, ops.projective_icp_tape_bytes(c.numiters)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(c.stride, c.numiters, c.kw["damp"], c.kw["dist_thresh"],
                                                        c.kw["angle_thresh"]), huber_k=c.huber_k)
    T, _, scale = ops._picp_solve(opt, b("vertex"), b("normal"), b("depth"), b("K"), b("index"), b("model_pose"), maps,
                                  b("T0"), tapes=tapes, return_trace=True, return_scale=True)
    assert np.array_equal(bits(host(T[0])), bits(c.assoc.pose))
    # the tape row holds the iteration's threshold in pad[0] (byte 312 of 328)
    taped = host(tapes).reshape(c.numiters, 328)[:, 312:316].copy().view(F).reshape(-1)
    assert np.array_equal(bits(taped), bits(c.assoc.deltas)) and np.array_equal(bits(host(scale[0])), bits(taped))
    vb, rows_, ib = ops.projective_icp_backward_batch(b("vertex"), b("normal"), b("depth"), b("K"), b("index"),
                                                      b("model_pose"), maps, tapes, dev(c.T_bar)[None], huber_k=c.huber_k,
                                                      **kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(vb[0])), bits(got[0])) and np.array_equal(bits(host(ib[0])), bits(got[3]))
    assert bc.rel_err(host(rows_[0][0]), got[1]) <= MAP_BOUND and bc.rel_err(host(rows_[0][1]), got[2]) <= MAP_BOUND
    # the constant-threshold backward with the first iteration's threshold is another function: the tape is read
    cvb, _, _ = ops.projective_icp_backward_batch(b("vertex"), b("normal"), b("depth"), b("K"), b("index"),
                                                  b("model_pose"), maps, tapes, dev(c.T_bar)[None],
                                                  huber_delta=float(c.assoc.deltas[0]), **kw)
    assert bc.rel_err(host(cvb[0]), got[0]) > 1e-3


# ------------------------------------------------------------------------------------------ 5. provider and drivers
SEEDS = (0, 1)


@pytest.fixture(scope="module")
def sequences():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(L, H, W, seed=s) for s in SEEDS]


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_equal_the_hand_written_loop(gs, ops, sequences, which):
    want = hand_written_loop(gs, ops, which, frames_of(gs, sequences), huber_k=K)
    const = hand_written_loop(gs, ops, which, frames_of(gs, sequences), huber_delta=0.005)
    assert not np.array_equal(host(want[1]), host(const[1]))                  # the rule reaches the solve
    same_run(make_slam(gs, which, huber_k=K)(frames_of(gs, sequences)), want)
    # on the autograd tape (inputs that do not require grad): the same bits
    taped = make_slam(gs, which, huber_k=K, odom_differentiable=True)(frames_of(gs, sequences))
    same_run(taped, want)


def test_driver_with_the_colour_term_equals_the_hand_written_loop(gs, ops):
    kw = dict(huber_k=K, color_huber_delta=COLOR_DELTA)
    want = hand_written_loop(gs, ops, "PointFusion", textured_frames(gs), weight=1.0, **kw)
    const = hand_written_loop(gs, ops, "PointFusion", textured_frames(gs), weight=1.0, huber_delta=0.005,
                              color_huber_delta=COLOR_DELTA)
    assert not np.array_equal(host(want[1]), host(const[1]))
    same_run(make_slam(gs, "PointFusion", color_weight=1.0, **kw)(textured_frames(gs)), want)


def test_gradients_reach_the_sensor_depth(gs, sequences):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from tests.test_hip_picp_backward import two_frame_map
    prov = ProjectiveICPOdometryProvider(numiters=5, stride=2, differentiable=True, huber_k=K)
    frames, pc_ = two_frame_map(gs, sequences)
    live = frames[:, 2]
    live.depth_image.requires_grad_(True)
    prev = frames.poses[:, 1:2].clone().requires_grad_(True)
    T = prov.localize(pc_, live, prev)
    assert T.grad_fn is not None
    plain = ProjectiveICPOdometryProvider(numiters=5, stride=2, huber_k=K).localize(pc_, frames[:, 2], prev.detach())
    none = ProjectiveICPOdometryProvider(numiters=5, stride=2).localize(pc_, frames[:, 2], prev.detach())
    assert np.array_equal(bits(host(T)), bits(host(plain))) and not np.array_equal(host(plain), host(none))
    T[:, 0, :3, 3].sum().backward()
    for g in (live.depth_image.grad, prev.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
