"""GPU tests of the projective ICP's per-pixel weights (gs_picp.hip / gs_picp_color.hip / gs_picp_scale.hip /
gs_picp_bwd.hip -> the gs_projective_icp_*weighted* entries -> ops.projective_icp*(pixel_weights=...) /
WeightedProjectiveICPFunction -> ProjectiveICPOdometryProvider(pixel_weights=f) -> ICPSLAM / PointFusion(
odom_pixel_weights=f)), held bit for bit to the NumPy restatement (tests/picp_weighted_ref.py) at the smallest shapes
that can go wrong:

    17 x 31, stride 1   527 slots: two full chunks and a tail of 15; "cover" masks a whole wave (slots 0 .. 63), a whole
                        chunk (256 .. 511) and the tail (512 .. 526); "special" scatters 0, -0, -1, NaN, +-inf, a denormal
                        and 2^-20 .. 2^20
    17 x 31, stride 3   66 slots, one partial chunk, special weights
    17 x 31, stride 3   (backward) random weights in [0.25, 2] with the first four rows masked
    60 x 80, strides 1 and 4   the moved-block scenes, random weights with the block masked
    B = 3 with the middle sequence's weights NULL, B = 9 past one launch group of 8

The backward is held to the float64 adjoint within kernel_bound(gap) of tests/backward_cases.py, gap the float32-vs-float64
distance of that NumPy adjoint on the same case (no bound comes from a kernel's output), and to EQUAL BITS between runs
and between the atomic and the ordered mode wherever the contract says so."""
import math

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_color_ref as pcr
from tests import picp_grad_ref as gr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_weighted_ref as wr
from tests.test_hip_picp import FUSION, bits, dev, frames_of, host, map_rows, three_sequences

pytestmark = pytest.mark.gpu

DELTA, COLOR_DELTA, WEIGHT, K_HUBER = 0.005, 0.02, 0.2, 1.345
GEO = {"plain": dict(), "delta": dict(huber_delta=DELTA), "k": dict(huber_k=K_HUBER, huber_delta=0.001)}
JOINT = {"plain": dict(), "delta": dict(huber_delta=DELTA, color_huber_delta=COLOR_DELTA),
         "ck": dict(color_huber_k=K_HUBER, color_huber_delta=0.005),
         "both": dict(huber_k=K_HUBER, huber_delta=0.001, color_huber_k=K_HUBER)}
SHAPES = [(17, 31, 1, "cover"), (17, 31, 1, "special"), (17, 31, 3, "special"), (60, 80, 1, "block"), (60, 80, 4, "block")]
NUMITERS = 4
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


_FX = {}


def fixture(h, w, kind, color=False):
    """(fixture, weights (h, w) float32): cached and read-only"""
    key = (h, w, kind, color)
    if key not in _FX:
        fx = pcr.textured_fixture(h, w, scene="plane") if color else pr.convergence_fixture(h, w)
        if kind == "block":
            fx = rr.moved_block(fx)
            wts = wr.random_weights((h, w), patch=rr.BLOCK)
        elif kind == "special":
            wts = wr.special_weights((h, w))
        elif kind == "patch":
            wts = wr.random_weights((h, w), patch=(slice(0, 4), slice(0, w)))
        else:
            wts = wr.random_weights((h, w))
            flat = wts.reshape(-1)
            flat[0:64], flat[256:] = 0, 0
        wts.setflags(write=False)
        _FX[key] = (fx, wts)
    return _FX[key]


def same(got, want):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def geo_args(fx):
    return [dev(fx[k]) for k in pr.ARGS[:-1]]


def color_args(fx):
    return [dev(fx[k]) for k in ("color", "model")]


# ------------------------------------------------------------------------------------------ 1. forward against the restatement
@pytest.mark.parametrize("which", sorted(GEO))
@pytest.mark.parametrize("h,w,stride,kind", SHAPES)
def test_solve_and_rows_bit_for_bit(ops, h, w, stride, kind, which):
    fx, wts = fixture(h, w, kind)
    kw = GEO[which]
    want = wr.solve(*pr.args_of(fx), wts, fx["T0"], stride=stride, numiters=NUMITERS, **kw)
    T, trace, scale = ops.projective_icp(*geo_args(fx), dev(fx["T0"]), stride=stride, numiters=NUMITERS, return_trace=True,
                                         return_scale=True, pixel_weights=dev(wts), **kw)
    assert same(T, want[0]) and same(trace, want[1]) and same(scale, want[2]), (host(T), want[0])
    assert want[1][-1, 0] > 20 and np.isfinite(want[0]).all()
    # the tables, at the pose the solve ended at
    r = wr.rows(*pr.args_of(fx), wts, want[0], stride=stride, **kw)
    assert (r.code == wr.MASKED).any() and r.count > 20
    got = ops.projective_icp_rows(*geo_args(fx), dev(want[0]), stride=stride, pixel_weights=dev(wts), return_weights=True,
                                  **kw)
    rows_, weight = got[0], got[1]
    assert np.array_equal(host(rows_.code), r.code), np.nonzero(host(rows_.code) != r.code)
    assert np.array_equal(host(rows_.row), r.row) and same(rows_.a, r.a) and same(rows_.b, r.b)
    assert same(rows_.sums, r.sums) and int(rows_.count) == r.count and same(weight, r.weight)
    if "huber_k" in kw:
        assert same(got[2], np.array([r.delta], np.float32))
    only = ops.projective_icp_rows(*geo_args(fx), dev(want[0]), stride=stride, pixel_weights=dev(wts), **kw)
    assert isinstance(only, ops.ProjectiveRows) and same(only.sums, r.sums)


@pytest.mark.parametrize("which", sorted(JOINT))
@pytest.mark.parametrize("h,w,stride,kind", [(17, 31, 1, "cover"), (17, 31, 3, "special"), (60, 80, 4, "block")])
def test_joint_solve_and_rows_bit_for_bit(ops, h, w, stride, kind, which):
    fx, wts = fixture(h, w, kind, color=True)
    kw = JOINT[which]
    want = wr.color_solve(*pcr.args_of(fx), wts, fx["T0"], WEIGHT, stride=stride, numiters=3, **kw)
    T, trace, scale, cscale = ops.projective_icp_color(*geo_args(fx), dev(fx["T0"]), *color_args(fx), color_weight=WEIGHT,
                                                       stride=stride, numiters=3, return_trace=True, return_scale=True,
                                                       return_color_scale=True, pixel_weights=dev(wts), **kw)
    assert same(T, want[0]) and same(trace, want[1]) and same(scale, want[2]) and same(cscale, want[3])
    assert (want[1][:, 8] > 5).all()
    r = wr.color_rows(*pcr.args_of(fx), wts, want[0], WEIGHT, stride=stride, **kw)
    got = ops.projective_icp_color_rows(*geo_args(fx), dev(want[0]), *color_args(fx), color_weight=WEIGHT, stride=stride,
                                        pixel_weights=dev(wts), return_weights=True, **kw)
    q = got[0]
    assert np.array_equal(host(q.code), r.code) and np.array_equal(host(q.row), r.row)
    assert np.array_equal(host(q.colored) != 0, r.colored) and not r.colored[r.code == wr.MASKED].any()
    for k in ("a", "b", "ac", "bc", "sums"):
        assert same(getattr(q, k), getattr(r, k)), k
    assert int(q.count) == r.count and int(q.color_count) == r.color_count
    assert same(got[1], r.weight) and same(got[2], r.color_weight)
    if "huber_k" in kw or "color_huber_k" in kw:
        assert same(got[3], np.array([r.delta], np.float32)) and same(got[4], np.array([r.cdelta], np.float32))


# ------------------------------------------------------------------------------------------ 2. all ones = unweighted
def taped(ops, fx, stride, weights, huber_delta=0.0, huber_k=0.0):
    """(pose, trace, thresholds, tape bytes) of the taped solve, with pixel weights or through the unweighted entry"""
    b = lambda k: dev(fx[k]).unsqueeze(0)      # noqa: E731
    tapes = torch.zeros((1, ops.projective_icp_tape_bytes(NUMITERS)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(stride, NUMITERS, 1e-8, 0.1, 30.0), huber_delta=huber_delta,
                            huber_k=huber_k)
    w = None if weights is None else [dev(weights)]
    res = ops._picp_solve(opt, b("vertex"), b("normal"), b("depth"), b("K"), b("index"), b("model_pose"),
                          [(dev(fx["points"]), dev(fx["normals"]), None, None)], b("T0"), tapes=tapes, weights=w,
                          return_trace=True, return_scale=True)
    torch.cuda.synchronize()
    return [host(x) for x in res] + [host(tapes)]


@pytest.mark.parametrize("which", sorted(GEO))
@pytest.mark.parametrize("h,w,stride,kind", [(17, 31, 1, "cover"), (17, 31, 3, "special"), (60, 80, 4, "block")])
def test_all_ones_has_the_bits_of_the_unweighted_entry_tape_included(ops, h, w, stride, kind, which):
    fx, _ = fixture(h, w, kind)
    got = taped(ops, fx, stride, np.ones((h, w), np.float32), **GEO[which])
    want = taped(ops, fx, stride, None, **GEO[which])
    for g, x in zip(got, want):
        assert g.shape == x.shape and g.tobytes() == x.tobytes()
    assert np.frombuffer(want[3].tobytes(), np.int64).reshape(NUMITERS, 41)[:, 40].min() > 20      # the taped counts


JOINT_SHAPES = [(17, 31, 1, "cover"), (17, 31, 3, "special"), (60, 80, 4, "block")]


@pytest.mark.parametrize("which", sorted(JOINT))
@pytest.mark.parametrize("h,w,stride,kind", JOINT_SHAPES)
def test_all_ones_has_the_bits_of_the_unweighted_joint_entry(ops, h, w, stride, kind, which):
    """(the joint solve has no tape: pose, trace and both threshold tables)"""
    fx, _ = fixture(h, w, kind, color=True)
    kw = dict(color_weight=WEIGHT, stride=stride, numiters=3, return_trace=True, return_scale=True,
              return_color_scale=True, **JOINT[which])
    got = ops.projective_icp_color(*geo_args(fx), dev(fx["T0"]), *color_args(fx), pixel_weights=torch.ones(h, w).cuda(),
                                   **kw)
    want = ops.projective_icp_color(*geo_args(fx), dev(fx["T0"]), *color_args(fx), **kw)
    for g, x in zip(got, want):
        assert same(g, host(x))
    assert (host(want[1])[:, 8] > 5).all()


# ------------------------------------------------------------------------------------------ 3. a mask = a zeroed depth
@pytest.mark.parametrize("which", sorted(GEO))
@pytest.mark.parametrize("h,w,stride,kind", [(17, 31, 1, "cover"), (17, 31, 3, "special"), (60, 80, 1, "block"),
                                             (60, 80, 4, "block")])
def test_a_mask_has_the_bits_of_a_zeroed_depth(ops, h, w, stride, kind, which):
    fx, wts = fixture(h, w, kind)
    mask = np.where(wr.masks(wts), np.float32(0), np.float32(1))
    zfx = wr.zeroed_depth(fx, mask)
    kw = dict(stride=stride, numiters=NUMITERS, return_trace=True, return_scale=True, **GEO[which])
    got = ops.projective_icp(*geo_args(fx), dev(fx["T0"]), pixel_weights=dev(mask), **kw)
    want = ops.projective_icp(*geo_args(zfx), dev(fx["T0"]), **kw)
    for g, x in zip(got, want):
        assert same(g, host(x))
    r = ops.projective_icp_rows(*geo_args(fx), dev(fx["T0"]), stride=stride, pixel_weights=dev(mask), **GEO[which])
    z = ops.projective_icp_rows(*geo_args(zfx), dev(fx["T0"]), stride=stride, **GEO[which])
    rc_, zc = host(r.code), host(z.code)
    assert ((rc_ != zc) == ((rc_ == wr.MASKED) & (zc == 1))).all() and (rc_ == wr.MASKED).any()
    for k in ("row", "a", "b", "sums", "count"):
        assert same(getattr(r, k), host(getattr(z, k))), k


@pytest.mark.parametrize("which", sorted(JOINT))
@pytest.mark.parametrize("h,w,stride,kind", JOINT_SHAPES)
def test_a_mask_has_the_bits_of_a_zeroed_depth_in_the_joint_solve(ops, h, w, stride, kind, which):
    fx, wts = fixture(h, w, kind, color=True)
    mask = np.where(wr.masks(wts), np.float32(0), np.float32(1))
    zfx = wr.zeroed_depth(fx, mask)
    kw = dict(color_weight=WEIGHT, stride=stride, numiters=3, return_trace=True, return_scale=True,
              return_color_scale=True, **JOINT[which])
    got = ops.projective_icp_color(*geo_args(fx), dev(fx["T0"]), *color_args(fx), pixel_weights=dev(mask), **kw)
    want = ops.projective_icp_color(*geo_args(zfx), dev(fx["T0"]), *color_args(zfx), **kw)
    for g, x in zip(got, want):
        assert same(g, host(x))
    assert (host(want[1])[:, 8] > 5).all()
    rkw = dict(color_weight=WEIGHT, stride=stride, **JOINT[which])
    r = ops.projective_icp_color_rows(*geo_args(fx), dev(fx["T0"]), *color_args(fx), pixel_weights=dev(mask), **rkw)
    z = ops.projective_icp_color_rows(*geo_args(zfx), dev(fx["T0"]), *color_args(zfx), **rkw)
    rc_, zc = host(r.code), host(z.code)
    assert ((rc_ != zc) == ((rc_ == wr.MASKED) & (zc == 1))).all() and (rc_ == wr.MASKED).any()
    for k in ("row", "a", "b", "ac", "bc", "colored", "sums", "count", "color_count"):
        assert same(getattr(r, k), host(getattr(z, k))), k


# ------------------------------------------------------------------------------------------ 4. batches
def batch_weights(seqs):
    return [wr.random_weights(q["depth"].shape, seed=20 + i, patch=(slice(5 * i, 5 * i + 12), slice(10, 40)))
            for i, q in enumerate(seqs)]


def batch_call(ops, seqs, weights, **kw):
    st = lambda k: torch.stack([dev(q[k]) for q in seqs])   # noqa: E731
    maps = [(dev(q["points"]), dev(q["normals"]), None, None, None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in seqs]
    return ops.projective_icp_batch(st("vertex"), st("normal"), st("depth"), st("K"), st("index"), st("model_pose"), maps,
                                    st("T0"), return_trace=True, pixel_weights=weights, **kw)


def test_batch_of_three_with_the_middle_weights_null(ops):
    seqs = three_sequences()
    wts = batch_weights(seqs)
    kw = dict(stride=2, numiters=5, huber_k=K_HUBER)
    T, trace = batch_call(ops, seqs, [dev(wts[0]), None, dev(wts[2])], **kw)
    for b, (q, w) in enumerate(zip(seqs, (wts[0], None, wts[2]))):
        want = wr.solve(*pr.args_of(q), w, q["T0"], **kw)
        assert same(T[b], want[0]) and same(trace[b], want[1]), b
    # as one tensor: every sequence has weights
    T3, trace3 = batch_call(ops, seqs, torch.stack([dev(x) for x in wts]), **kw)
    assert same(T3[0], host(T[0])) and same(T3[2], host(T[2])) and not same(T3[1], host(T[1]))
    want = wr.solve(*pr.args_of(seqs[1]), wts[1], seqs[1]["T0"], **kw)
    assert same(T3[1], want[0]) and same(trace3[1], want[1])


def test_batch_of_nine_crosses_the_launch_group(ops):
    seqs = three_sequences()
    wts = batch_weights(seqs)
    kw = dict(stride=4, numiters=4, huber_delta=DELTA)
    nine = [seqs[i % 3] for i in range(9)]
    w9 = [None if i == 7 else dev(wts[i % 3]) for i in range(9)]
    T, trace = batch_call(ops, nine, w9, **kw)
    for i in range(9):
        want = wr.solve(*pr.args_of(nine[i]), None if i == 7 else wts[i % 3], nine[i]["T0"], **kw)
        assert same(T[i], want[0]) and same(trace[i], want[1]), i
    assert (host(trace)[:, -1, 0] > 20).all()


# ------------------------------------------------------------------------------------------ 5. backward
BWD = {"s1_cover_delta": (17, 31, 1, "cover", dict(huber_delta=DELTA)),
       "s3_patch": (17, 31, 3, "patch", dict()),     # (not "special": weights over twelve decades on 30 slots leave the
                                                     # float32 yardstick, and with it the bound, without meaning)
       "s4_block_k": (60, 80, 4, "block", dict(huber_k=K_HUBER)),
       "s1_block_delta": (60, 80, 1, "block", dict(huber_delta=DELTA))}
T_BAR = bc.weights((4, 4), 31)


def leaves(fx, wts, grad=True):
    t = {k: dev(fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals", "T0")}
    t["w"] = dev(wts)
    for k in ("vertex", "points", "normals", "T0", "w"):
        t[k].requires_grad_(grad)
    return t


def run(ops, fx, wts, stride, deterministic, weighted=True, want_w=True, **kw):
    """differentiable solve and its backward: (pose, [vertex_bar, points_bar, normals_bar, T0_bar, w_bar])"""
    t = leaves(fx, wts)
    t["w"].requires_grad_(want_w)
    T = ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                           t["normals"], t["T0"], stride=stride, numiters=NUMITERS, differentiable=True,
                           deterministic=deterministic, pixel_weights=t["w"] if weighted else None, **kw)
    assert T.grad_fn is not None
    T.backward(dev(T_BAR))
    torch.cuda.synchronize()
    return host(T), [None if t[k].grad is None else host(t[k].grad) for k in ("vertex", "points", "normals", "T0", "w")]


def reference(fx, wts, stride, kw, dtype=np.float64):
    assoc = wr.association(*pr.args_of(fx), wts, fx["T0"], stride=stride, numiters=NUMITERS, **kw)
    wp = np.where(wr.masks(assoc.wp), np.float32(0), assoc.wp)        # (never read: masked slots are not used)
    vb, Pb, Nb, Tb, wb = wr.adjoint(gr.lattice(fx["vertex"], stride), fx["points"], fx["normals"], wp, assoc, fx["T0"],
                                    T_BAR, poses=assoc.poses, dtype=dtype)
    shape = fx["depth"].shape
    return assoc, [wr.on_image(vb, shape, stride), Pb, Nb, Tb, wr.on_image(wb, shape, stride)]


@pytest.mark.parametrize("name", sorted(BWD))
def test_backward_against_the_float64_adjoint_and_its_bits(ops, name):
    h, w, stride, kind, kw = BWD[name]
    fx, wts = fixture(h, w, kind)
    assoc, want = reference(fx, wts, stride, kw)
    _, want32 = reference(fx, wts, stride, kw, np.float32)
    gaps = [bc.rel_err(a, b) for a, b in zip(want32, want)]
    assert assoc.used.any(1).all() and (assoc.codes == wr.MASKED).any()
    T, atomic = run(ops, fx, wts, stride, False, **kw)
    assert same(T, assoc.pose), "the taped weighted forward left the restated solve"
    _, again = run(ops, fx, wts, stride, False, **kw)
    _, ordered = run(ops, fx, wts, stride, True, **kw)
    _, ordered2 = run(ops, fx, wts, stride, True, **kw)
    names = ("vertex_bar", "points_bar", "normals_bar", "init_pose_bar", "pixel_weights_bar")
    for out, g, x, gap in zip(names, atomic, want, gaps):
        assert g.shape == x.shape and np.isfinite(g).all(), (name, out)
        print("%s %s: rel_err %.3g, bound %.3g (gap %.2g)" % (name, out, bc.rel_err(g, x), bc.kernel_bound(gap), gap))
    for out, g, x, gap in zip(names, atomic, want, gaps):
        assert bc.rel_err(g, x) <= bc.kernel_bound(gap), (name, out, bc.rel_err(g, x), bc.kernel_bound(gap))
    for i in (0, 3, 4):     # bitwise reproducible: between runs and between the two modes
        assert same(atomic[i], again[i]) and same(atomic[i], ordered[i]) and same(ordered[i], ordered2[i]), names[i]
    for i in (1, 2):        # the map gradients: equal bits under deterministic=True, float64 atomics otherwise
        assert same(ordered[i], ordered2[i]), names[i]
        assert bc.rel_err(atomic[i], again[i]) <= MAP_BOUND and bc.rel_err(ordered[i], want[i]) <= bc.kernel_bound(gaps[i])
    # +0.0 off the lattice, at masked pixels and at pixels never used
    wb = atomic[4]
    never = np.ones((h, w), bool)
    never[::stride, ::stride] = ~wr.on_image(assoc.used.any(0), (h, w), stride)[::stride, ::stride]
    assert (bits(wb[never]) == 0).all() and wr.masks(wts)[::stride, ::stride].any() and np.abs(wb).max() > 0


@pytest.mark.parametrize("which", sorted(GEO))
def test_backward_with_all_ones_has_the_bits_of_the_unweighted_backward(ops, which):
    fx, _ = fixture(60, 80, "block")
    ones = np.ones((60, 80), np.float32)
    for deterministic in (False, True):
        T, got = run(ops, fx, ones, 4, deterministic, **GEO[which])
        T0, want = run(ops, fx, ones, 4, deterministic, weighted=False, **GEO[which])
        assert same(T, T0) and want[4] is None and np.abs(got[4]).max() > 0
        for i in (0, 3) + ((1, 2) if deterministic else ()):
            assert same(got[i], want[i]), (deterministic, i)
        if not deterministic:
            assert bc.rel_err(got[1], want[1]) <= MAP_BOUND and bc.rel_err(got[2], want[2]) <= MAP_BOUND


def test_outputs_not_asked_for(ops):
    fx, wts = fixture(60, 80, "block")
    _, full = run(ops, fx, wts, 4, True, huber_delta=DELTA)
    _, part = run(ops, fx, wts, 4, True, want_w=False, huber_delta=DELTA)
    assert part[4] is None
    for i in range(4):
        assert same(part[i], full[i]), i
    # the tensor-level call
    b = lambda k: dev(fx[k]).unsqueeze(0)      # noqa: E731
    args = [b(k) for k in ("vertex", "normal", "depth", "K", "index", "model_pose")]
    maps = [(dev(fx["points"]), dev(fx["normals"]), None, None)]
    tapes = torch.empty((1, ops.projective_icp_tape_bytes(NUMITERS)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(4, NUMITERS, 1e-8, 0.1, 30.0), huber_delta=DELTA)
    ops._picp_solve(opt, *args, maps, b("T0"), tapes=tapes, weights=[dev(wts)])
    kw = dict(stride=4, numiters=NUMITERS, huber_delta=DELTA, pixel_weights=dev(wts)[None])
    res = ops.projective_icp_backward_batch(*args, maps, tapes, dev(T_BAR)[None], want_pixel_weights=False, **kw)
    assert len(res) == 4 and res[3] is None and same(res[0][0], full[0])
    res = ops.projective_icp_backward_batch(*args, maps, tapes, dev(T_BAR)[None], want_pixel_weights=True,
                                            want_vertex=False, want_init=False, want_maps=[(False, False)], **kw)
    assert res[0] is None and res[2] is None and res[1] == [(None, None)] and same(res[3][0], full[4])


def test_backward_with_special_weights_is_reproducible_and_leaves_masked_pixels_alone(ops):
    """weights of 0, -0, -1, NaN, +-inf, a denormal and 2^-20 .. 2^20 (no float64 bound means anything on that system:
    the claims that need none): equal bits between runs and between the modes, +0.0 at every pixel that is masked"""
    for stride in (1, 3):
        fx, wts = fixture(17, 31, "special")
        _, atomic = run(ops, fx, wts, stride, False, huber_delta=DELTA)
        _, again = run(ops, fx, wts, stride, False, huber_delta=DELTA)
        _, ordered = run(ops, fx, wts, stride, True, huber_delta=DELTA)
        _, ordered2 = run(ops, fx, wts, stride, True, huber_delta=DELTA)
        for i in (0, 3, 4):
            assert same(atomic[i], again[i]) and same(atomic[i], ordered[i]) and same(ordered[i], ordered2[i]), (stride, i)
        for i in (1, 2):
            assert same(ordered[i], ordered2[i]), (stride, i)
        wb = atomic[4]
        off = np.ones((17, 31), bool)
        off[::stride, ::stride] = False
        assert np.isfinite(wb).all() and (bits(wb[wr.masks(wts) | off]) == 0).all() and np.abs(wb).max() > 0
        assert all(np.isfinite(g).all() for g in atomic)


@pytest.mark.parametrize("deterministic", [False, True])
def test_backward_with_a_null_weights_entry(ops, deterministic):
    """B = 3 in list form, the middle sequence without weights (its pointer is NULL) and its pixel_weights_bar asked for:
    every sequence has the bits of its own call, the middle one those of its call with weights of all ones"""
    seqs = three_sequences()
    wts = batch_weights(seqs)
    wts[1] = np.ones_like(wts[1])
    st = lambda k: torch.stack([dev(q[k]) for q in seqs])   # noqa: E731
    args = [st(k) for k in ("vertex", "normal", "depth", "K", "index", "model_pose")]
    maps = [(dev(q["points"]), dev(q["normals"]), None,
             None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")) for q in seqs]
    given = [dev(wts[0]), None, dev(wts[2])]
    tapes = torch.empty((3, ops.projective_icp_tape_bytes(NUMITERS)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(4, NUMITERS, 1e-8, 0.1, 30.0), huber_delta=DELTA)
    T = ops._picp_solve(opt, *args, maps, st("T0"), tapes=tapes, weights=given)
    vb, rows_, ib, wb = ops.projective_icp_backward_batch(*args, maps, tapes, dev(T_BAR)[None].repeat(3, 1, 1), stride=4,
                                                          numiters=NUMITERS, huber_delta=DELTA, pixel_weights=given,
                                                          want_pixel_weights=True, deterministic=deterministic)
    torch.cuda.synchronize()
    for b, q in enumerate(seqs):
        t = leaves(q, wts[b])
        n_dev = None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")
        Ts = ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                                t["normals"], t["T0"], n_dev=n_dev, pixel_weights=t["w"], stride=4, numiters=NUMITERS,
                                huber_delta=DELTA, differentiable=True, deterministic=deterministic)
        Ts.backward(dev(T_BAR))
        assert same(T[b], host(Ts)) and same(vb[b], host(t["vertex"].grad)) and same(ib[b], host(t["T0"].grad)), b
        assert same(wb[b], host(t["w"].grad)) and host(wb[b]).any(), b
        if deterministic:
            assert same(rows_[b][0], host(t["points"].grad)) and same(rows_[b][1], host(t["normals"].grad)), b


def test_backward_of_a_batch_of_nine(ops):
    """past one launch group: every sequence has the bits of its own call"""
    seqs = three_sequences()
    wts = batch_weights(seqs)
    st = lambda k: torch.stack([dev(seqs[i % 3][k]) for i in range(9)])   # noqa: E731
    vertex, w9 = st("vertex").requires_grad_(True), torch.stack([dev(wts[i % 3]) for i in range(9)]).requires_grad_(True)
    maps = [(dev(seqs[i % 3]["points"]), dev(seqs[i % 3]["normals"]), None,
             None if seqs[i % 3]["n_dev"] is None else torch.tensor([seqs[i % 3]["n_dev"]], dtype=torch.int64,
                                                                   device="cuda")) for i in range(9)]
    kw = dict(stride=4, numiters=NUMITERS, huber_delta=DELTA, differentiable=True)
    T = ops.projective_icp_batch(vertex, st("normal"), st("depth"), st("K"), st("index"), st("model_pose"), maps, st("T0"),
                                 pixel_weights=w9, **kw)
    T.backward(dev(T_BAR)[None].repeat(9, 1, 1))
    torch.cuda.synchronize()
    for i in range(9):
        q = seqs[i % 3]
        t = leaves(q, wts[i % 3])
        n_dev = None if q["n_dev"] is None else torch.tensor([q["n_dev"]], dtype=torch.int64, device="cuda")
        Ts = ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                                t["normals"], t["T0"], n_dev=n_dev, pixel_weights=t["w"], **kw)
        Ts.backward(dev(T_BAR))
        assert same(T[i], host(Ts)) and same(vertex.grad[i], host(t["vertex"].grad)), i
        assert same(w9.grad[i], host(t["w"].grad)) and host(w9.grad[i]).any(), i


# ------------------------------------------------------------------------------------------ 6. provider and drivers
LD, SEEDS = 4, (0, 1)
KW = dict(dsratio=2, numiters=6)


@pytest.fixture(scope="module")
def sequences():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(LD, 60, 80, seed=s) for s in SEEDS]


def column_mask(frames):
    """the weights of the driver tests: the sensor model, with a band of columns masked"""
    from gradslam_amd.odometry import axial_noise_weights
    w = axial_noise_weights(frames).clone()
    w[..., 30:45] = 0
    return w


def hand_written_loop(gs, ops, which, frames, f, flt=None, **kw):
    """render the map at the previous pose, solve from that pose with the weights of the frame, update the map"""
    from gradslam_amd.slam.fusionutils import update_map_aggregate, update_map_fusion
    B = frames.shape[0]
    pc = gs.Pointclouds(device="cuda")
    out, prev, calls = [], None, 0
    K = frames.intrinsics[:, 0].contiguous()
    for s in range(LD):
        live = frames[:, s]
        if flt is not None:
            live = live.bilateral_filter(**flt)
        if s > 0:
            maps = [(pc._buf["points"][b], pc._buf["normals"][b], None, None) + tuple(pc._count_of(b)) for b in range(B)]
            if which == "PointFusion":
                _, extras = pc.render(frames.intrinsics, prev.view(B, 1, 4, 4), 60, 80, return_extras=True)
                index = extras["index"][:, 0]
            else:
                index = ops.render_map_batch(maps, prev.view(B, 1, 4, 4), K, 60, 80).index[:, 0]
            fr = live.to_channels_last()
            pose = ops.projective_icp_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K,
                                            index, prev, maps, prev, pixel_weights=f(live).reshape(B, 60, 80), **kw)
            calls += 1
            live.poses = pose.view(B, 1, 4, 4)
        if which == "PointFusion":
            pc = update_map_fusion(pc, live, FUSION["dist_th"], math.cos(FUSION["angle_th"] * math.pi / 180),
                                   FUSION["sigma"], inplace=True)
        else:
            pc = update_map_aggregate(pc, live, inplace=True)
        prev = live.poses[:, 0].contiguous()
        out.append(prev.clone())
    return pc, torch.stack(out, 1), calls


def run_steps(slam, gs, frames, inplace):
    pc = gs.Pointclouds(device="cuda")
    prev, out = None, []
    for s in range(LD):
        live = frames[:, s]
        pc, poses = slam.step(pc, live, prev, inplace=inplace)
        live.poses = poses
        prev = live
        out.append(poses[:, 0].clone())
    return pc, torch.stack(out, 1)


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_equal_the_hand_written_loop(gs, ops, sequences, which):
    calls = []

    def f(frames):
        calls.append(tuple(frames.shape))
        return column_mask(frames)

    cls = getattr(gs.slam, which)
    extra = dict(FUSION) if which == "PointFusion" else {}
    robust = dict(huber_k=K_HUBER)
    want_pc, want, n = hand_written_loop(gs, ops, which, frames_of(gs, sequences), column_mask, stride=KW["dsratio"],
                                         numiters=KW["numiters"], **robust)
    plain = cls(odom="projicp", device="cuda", **KW, **robust, **extra)(frames_of(gs, sequences))[1]
    assert n == LD - 1 and not np.array_equal(host(plain), host(want))
    for how in ("fast", "generic", "forward"):
        slam = cls(odom="projicp", device="cuda", odom_pixel_weights=f, **KW, **robust, **extra)
        del calls[:]
        if how == "forward":
            pc, poses = slam(frames_of(gs, sequences))
        else:
            pc, poses = run_steps(slam, gs, frames_of(gs, sequences), inplace=how == "fast")
        assert len(calls) == LD - 1 and all(c[:2] == (len(SEEDS), 1) for c in calls), (how, calls)   # once per localisation
        assert same(poses, host(want)), how
        for b in range(len(SEEDS)):
            for g, x in zip(map_rows(pc, b), map_rows(want_pc, b)):
                assert same(g, x), (how, b)
    # with a depth filter the callable sees the filtered copy
    flt = dict(radius=2, sigma_space=1.5, sigma_range=0.05)
    want_pc, want, _ = hand_written_loop(gs, ops, which, frames_of(gs, sequences), column_mask, flt=flt,
                                         stride=KW["dsratio"], numiters=KW["numiters"], **robust)
    slam = cls(odom="projicp", device="cuda", odom_pixel_weights=f, depth_filter=flt, **KW, **robust, **extra)
    pc, poses = run_steps(slam, gs, frames_of(gs, sequences), inplace=True)
    assert same(poses, host(want))
    for b in range(len(SEEDS)):
        for g, x in zip(map_rows(pc, b), map_rows(want_pc, b)):
            assert same(g, x), b


class Confidence(torch.nn.Module):
    """one parameter: the steepness of a depth-dependent confidence"""

    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(0.5))

    def forward(self, frames):
        z = frames.to_channels_last().depth_image[..., 0]
        return torch.where(z > 0, torch.exp(-self.k * (z - 1.0) ** 2), torch.zeros_like(z))


@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_a_module_behind_the_weights_gets_a_gradient(gs, sequences, which):
    net = Confidence().cuda()
    cls = getattr(gs.slam, which)
    extra = dict(FUSION) if which == "PointFusion" else {}
    slam = cls(odom="projicp", device="cuda", odom_pixel_weights=net, odom_differentiable=True, huber_delta=DELTA, **KW,
               **extra)
    frames = frames_of(gs, sequences)
    pc = gs.Pointclouds(device="cuda")
    prev = None
    for s in range(2):
        live = frames[:, s]
        pc, poses = slam.step(pc, live, prev, inplace=False)
        live.poses = poses
        prev = live
    assert poses.grad_fn is not None
    gt = torch.from_numpy(np.stack([q["poses"][1] for q in sequences])).cuda()
    loss = ((poses[:, 0, :3, 3] - gt[:, :3, 3]) ** 2).sum()
    loss.backward()
    g = float(net.k.grad)
    print("%s: d loss / d k = %.3e" % (which, g))
    assert math.isfinite(g) and g != 0.0
