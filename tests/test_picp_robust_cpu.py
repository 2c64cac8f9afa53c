"""CPU tests of the projective ICP's Huber weights: the NumPy restatement (tests/picp_robust_ref.py) -- its identity at
delta = 0, what the weights are for (a moved block inside the distance gate), its float64 adjoint against central
differences, the float32 yardsticks of tests/picp_robust_backward_cases.py and what the cases exercise -- and, without a
GPU, the exports, the argument checks of the C entry points (made before any HIP call) and of the Python layers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import backward_cases as bc
from tests import picp_color_ref as pcr
from tests import picp_ref as pr
from tests import picp_robust_backward_cases as rc
from tests import picp_robust_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1e-6     # what tests/test_picp_backward_cpu.py holds the plain adjoint to
# steps relative to the input's scale.  The weight delta / |b| is far more curved than the plain iteration (a residual of a
# few millimetres against a step of 1e-6 x 100 m, the vertex the cases move out of the view): the truncation error of a
# central difference falls with the square of the step (measured on edge_s1's map points: 4e-4 at 1e-6, 4e-6 at 1e-7, 4e-8
# at 3e-8) until the rounding of float64 takes over below 1e-8: half-decade steps from 1e-6 down, the best one counts
FD_STEPS = (1e-6, 3e-7, 1e-7, 3e-8, 1e-8)
DELTA, COLOR_DELTA, WEIGHT = 0.005, 0.02, 0.2
NEW = ("gs_projective_icp_robust_batch_f32", "gs_projective_icp_robust_rows_f32",
       "gs_projective_icp_robust_backward_batch_f32", "gs_projective_icp_color_robust_batch_f32",
       "gs_projective_icp_color_robust_rows_f32")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------ the restatement
def test_weights_are_the_pinned_float32_operations():
    b = np.array([0.0, 1e-3, -1e-3, 5e-3, -6e-3, 0.25, np.nan, -np.inf], np.float32)
    w = rr.slot_weights(b, DELTA)
    d = np.float32(DELTA)
    want = [1.0, 1.0, 1.0, 1.0, d / np.float32(6e-3), d / np.float32(0.25), 1.0, 0.0]
    assert w.dtype == np.float32 and np.array_equal(bits(w), bits(np.array(want, np.float32)))
    assert np.array_equal(rr.clipped(b, DELTA), [False, False, False, False, True, True, False, True])
    assert (rr.slot_weights(b, 0.0) == 1).all() and not rr.clipped(b, 0.0).any()      # 0 switches the weight off
    assert (rr.slot_weights(b, DELTA, np.zeros(8, bool)) == 0).all()
    # a term: the exact product, then one rounding by the weight
    a = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]], np.float32)
    bb = np.array([7e-3], np.float32)
    ww = rr.slot_weights(bb, DELTA)
    t = rr.terms(np.zeros(1, np.int32), a, bb, ww)
    assert t[0, 27] == float(ww[0]) * (float(bb[0]) * float(bb[0])) and t[0, 1] == float(ww[0]) * (float(a[0, 0]) * float(a[0, 1]))
    assert (rr.terms(np.ones(1, np.int32), a, bb, ww) == 0).all()


@pytest.mark.parametrize("stride", [1, 4])
def test_delta_zero_is_the_plain_restatement_bit_for_bit(stride):
    fx = pr.convergence_fixture()
    T, trace = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride)
    T0, trace0 = rr.solve(*pr.args_of(fx), fx["T0"], 0.0, stride=stride)
    assert np.array_equal(bits(T), bits(T0)) and np.array_equal(bits(trace), bits(trace0))
    r, r0 = pr.rows(*pr.args_of(fx), T, stride=stride), rr.rows(*pr.args_of(fx), T, 0.0, stride=stride)
    assert np.array_equal(bits(r.sums), bits(r0.sums)) and np.array_equal(r0.weight, (r.code == 0).astype(np.float32))
    cf = pcr.textured_fixture(scene="wave")
    Tc, tc = pcr.solve(*pcr.args_of(cf), cf["T0"], WEIGHT, stride=stride, numiters=4)
    Tc0, tc0 = rr.color_solve(*pcr.args_of(cf), cf["T0"], WEIGHT, 0.0, 0.0, stride=stride, numiters=4)
    assert np.array_equal(bits(Tc), bits(Tc0)) and np.array_equal(bits(tc), bits(tc0))


def test_weighted_rows_keep_the_rows_and_the_count():
    fx = rr.moved_block(pr.convergence_fixture())
    plain = pr.rows(*pr.args_of(fx), fx["T0"])
    r = rr.rows(*pr.args_of(fx), fx["T0"], DELTA)
    for k in ("code", "row", "a", "b"):
        assert np.array_equal(getattr(r, k), getattr(plain, k)), k
    assert r.count == plain.count
    used = r.code == 0
    assert (r.weight[~used] == 0).all() and (r.weight[used] > 0).all() and (r.weight <= 1).all()
    assert 100 < (r.weight[used] < 1).sum() < used.sum() - 100
    assert 0 < r.sums[27] < plain.sums[27]            # the weighted sum of squares


# ------------------------------------------------------------------------------------------ what the weights are for
def test_a_moved_block_inside_the_gate_pulls_the_plain_solve_not_the_robust_one():
    """The 60 x 80 wave fixture, frame 5 against frame 0's map, 10 iterations; the block [15:38, 20:51] of the live depth
    (15 % of the image) is 4 cm nearer, well inside the 10 cm gate.  Translation error against the ground truth by the
    restatement: stride 1: plain 18.68 mm, delta 5 mm 4.78 mm, delta 2 mm 2.00 mm; stride 2: 18.70 / 4.69 / 1.98 mm."""
    fx = rr.moved_block(pr.convergence_fixture())
    assert (fx["depth"] != pr.convergence_fixture()["depth"]).mean() > 0.13
    for stride in (1, 2):
        err = {}
        for d in (0.0, 0.005, 0.002):
            T, trace = rr.solve(*pr.args_of(fx), fx["T0"], d, stride=stride)
            err[d] = rr.translation_error(T, fx["gt"])
            assert np.isfinite(trace).all()
        print("moved block, stride %d: plain %.2f mm, delta 5 mm %.2f mm, delta 2 mm %.2f mm"
              % (stride, 1e3 * err[0.0], 1e3 * err[0.005], 1e3 * err[0.002]))
        assert err[0.005] < 0.5 * err[0.0]
        assert err[0.002] < err[0.005]


@pytest.mark.parametrize("cdelta", [0.0, COLOR_DELTA])
def test_the_joint_solve_gains_as_much(cdelta):
    """The textured plane with the same block moved, color_weight 0.2, against the same solve without thresholds.  By the
    restatement: 8.44 mm at delta 0; 0.99 mm at delta 5 mm, with and without a colour threshold of 0.02 (the block moves the
    depth, not the colours: the colour threshold clips rows of the first linearisations only)."""
    fx = rr.moved_block(pcr.textured_fixture(scene="plane"))
    T0, _ = rr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, 0.0, 0.0)
    T, trace = rr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, DELTA, cdelta)
    e0, e = rr.translation_error(T0, fx["gt"]), rr.translation_error(T, fx["gt"])
    print("textured moved block, colour delta %g: delta 0 %.2f mm, delta 5 mm %.2f mm" % (cdelta, 1e3 * e0, 1e3 * e))
    assert e < 0.5 * e0 and np.isfinite(trace).all() and (trace[:, 8] > 100).all()
    first = rr.color_rows(*pcr.args_of(fx), fx["T0"], WEIGHT, DELTA, cdelta)
    clipped = (first.color_weight < 1) & first.colored
    assert (first.color_weight[~first.colored] == 0).all()
    assert clipped.any() == (cdelta > 0)


def test_clean_data_loses_nothing():
    """the undisturbed fixture: plain 0.092 mm, delta 5 mm 0.078 mm (14 of 3 363 rows clipped at the end)"""
    fx = pr.convergence_fixture()
    Tp, _ = pr.solve(*pr.args_of(fx), fx["T0"])
    Tr, _ = rr.solve(*pr.args_of(fx), fx["T0"], DELTA)
    ep, er = rr.translation_error(Tp, fx["gt"]), rr.translation_error(Tr, fx["gt"])
    r = rr.rows(*pr.args_of(fx), Tr, DELTA)
    n_clip = int(((r.weight < 1) & (r.code == 0)).sum())
    print("clean: plain %.4f mm, delta 5 mm %.4f mm, %d of %d rows clipped" % (1e3 * ep, 1e3 * er, n_clip, r.count))
    assert er <= 1.5 * ep and n_clip < 0.01 * r.count


# ------------------------------------------------------------------------------------------ adjoint vs finite differences
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_adjoint_against_central_differences(name):
    """<adjoint, d> against central differences of the float64 weighted forward (the clip flags frozen, the weight
    delta / |b| differentiated) along a random direction of each of the four inputs; the best of three steps counts"""
    c = rc.build(name)
    fx = c.fx
    x = [c.v.astype(np.float64), fx["points"].astype(np.float64), fx["normals"].astype(np.float64),
         np.asarray(fx["T0"], np.float64)]
    Tb = c.T_bar.astype(np.float64)
    grads = rr.adjoint(*x[:3], c.assoc, x[3], Tb, c.delta)
    assert (grads[3][3] == 0).all()
    rng = np.random.default_rng(3)
    worst = 0.0
    for i, what in enumerate(rc.OUTPUTS):
        d = rng.standard_normal(x[i].shape)
        if i == 3:
            d[3] = 0.0
        d[~np.isfinite(x[i])] = 0.0
        want = float(np.sum(grads[i] * d))
        scale = float(np.nanmax(np.abs(x[i])))
        best = np.inf
        for h in FD_STEPS:
            hi, lo = list(x), list(x)
            hi[i], lo[i] = x[i] + h * scale * d, x[i] - h * scale * d
            f1, _ = rr.forward(*hi[:3], c.assoc, hi[3], c.delta)
            f0, _ = rr.forward(*lo[:3], c.assoc, lo[3], c.delta)
            fd = float(np.sum(Tb[:3] * (f1 - f0)[:3])) / (2 * h * scale)
            best = min(best, abs(fd - want) / abs(want))
        print("%s %s: <adjoint, d> = %.6g, best relative error %.2e" % (name, what, want, best))
        worst = max(worst, best)
    assert worst <= FD_BOUND, (name, worst)


def test_the_weighted_adjoint_differs_from_the_plain_one_and_equals_it_without_clipped_slots():
    from tests import picp_grad_ref as gr
    c = rc.build("conv_s4")
    P, N = c.fx["points"], c.fx["normals"]
    got = rr.adjoint(c.v, P, N, c.assoc, c.fx["T0"], c.T_bar, c.delta, poses=c.assoc.poses)
    plain = gr.adjoint(c.v, P, N, c.assoc, c.fx["T0"], c.T_bar, poses=c.assoc.poses)
    assert bc.rel_err(got[0], plain[0]) > 1e-2
    free = c.assoc._replace(clipped=np.zeros_like(c.assoc.clipped))
    same = rr.adjoint(c.v, P, N, free, c.fx["T0"], c.T_bar, c.delta, poses=c.assoc.poses)
    for a, b in zip(same, plain):
        assert bc.rel_err(a, b) < 1e-12


# ------------------------------------------------------------------------------------------ yardsticks and cases
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_committed_gap_is_current(name):
    """the float32 yardstick the GPU suite uses is what this machine measures, within DRIFT"""
    c = rc.build(name)
    rc.claims(c)
    got, want = rc.gaps(name), rc.GAP[name]
    print(name, got, want)
    for out, g, w in zip(rc.OUTPUTS, got, want):
        assert w / bc.DRIFT <= g <= w * bc.DRIFT, (name, out, g, w)


def test_cases_cover_what_the_kernel_can_get_wrong():
    assert set(rc.GAP) == set(rc.CASES) == set(rc.DELTA)
    chunks = {-(-rc.build(n).v.shape[0] // 256) for n in rc.CASES}
    assert {1, 2, 8, 19} <= chunks, chunks
    assert rc.build("edge_s1").v.shape[0] % 256 != 0 and rc.build("edge_s3").v.shape[0] == 234
    assert rc.build("stale_dc").device_count is not None
    assert all(rc.build(n).numiters >= 2 for n in rc.CASES)
    for n in rc.NO_INLIER:
        c = rc.build(n)
        assert not c.assoc.used.any() and not c.assoc.clipped.any() and (c.assoc.trace == 0).all()
        ref = rc.reference(c)
        assert np.array_equal(ref[3][:3], c.T_bar[:3].astype(np.float64)) and (ref[3][3] == 0).all()
        assert all((r == 0).all() for r in ref[:3])


# ------------------------------------------------------------------------------------------ the library
def test_new_symbols_are_declared_and_exported_at_abi_3():
    lib = _C.lib()
    assert set(NEW) <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays


def _seq(**kw):
    from tests.test_picp_color_cpu import _seq as color_seq
    return color_seq(**kw)


def _prm():
    return _C.PicpParams(4, 10, 1e-8, 0.1, 0.866)


BAD = [float("nan"), -1e-3, float("inf"), -float("inf")]


@pytest.mark.parametrize("bad", BAD)
def test_entry_points_reject_a_bad_threshold_before_any_hip_call(bad):
    lib = _C.lib()
    q, prm = _seq(), _prm()
    tapes = (C.c_void_p * 1)(0x800000)
    bseq = (_C.PicpBackwardSeq * 1)()
    calls = {
        "gs_projective_icp_robust_batch_f32":
            lambda d: lib.gs_projective_icp_robust_batch_f32(C.pointer(q.base), None, 1, 48, 64, prm, d, None),
        "gs_projective_icp_robust_rows_f32":
            lambda d: lib.gs_projective_icp_robust_rows_f32(C.pointer(q.base), 48, 64, 4, 0.1, 0.866, d, *([None] * 7),
                                                            None),
        "gs_projective_icp_robust_backward_batch_f32":
            lambda d: lib.gs_projective_icp_robust_backward_batch_f32(bseq, 1, 48, 64, prm, d, None),
        "gs_projective_icp_color_robust_batch_f32":
            lambda d: lib.gs_projective_icp_color_robust_batch_f32(C.pointer(q), 1, 48, 64, prm, 0.1, d, 0.0, None),
        "gs_projective_icp_color_robust_rows_f32":
            lambda d: lib.gs_projective_icp_color_robust_rows_f32(C.pointer(q), 48, 64, 4, 0.1, 0.866, 0.1, d, 0.0,
                                                                  *([None] * 12), None),
    }
    for name, call in calls.items():
        assert call(bad) == 1, name                           # GS_ERR_INVALID
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "huber_delta" in msg, msg
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(q.base), tapes, 1, 48, 64, prm, bad, None) == 1
    assert lib.gs_projective_icp_color_robust_batch_f32(C.pointer(q), 1, 48, 64, prm, 0.1, 0.0, bad, None) == 1
    assert "color_huber_delta" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_color_robust_rows_f32(C.pointer(q), 48, 64, 4, 0.1, 0.866, 0.1, 0.0, bad,
                                                       *([None] * 12), None) == 1
    assert "color_huber_delta" in lib.gs_last_error().decode()


def test_entry_points_keep_the_checks_of_their_plain_counterparts():
    lib = _C.lib()
    prm = _prm()
    name = "gs_projective_icp_robust_batch_f32"
    assert lib.gs_projective_icp_robust_batch_f32(None, None, 1, 48, 64, prm, DELTA, None) == 1
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(_seq(vertex=0).base), None, 1, 48, 64, prm, DELTA, None) == 1
    assert lib.gs_last_error().decode().startswith(name) and "NULL" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(_seq().base), None, 1, 0, 64, prm, DELTA, None) == 1
    bad = _C.PicpParams(0, 10, 1e-8, 0.1, 0.866)
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(_seq().base), None, 1, 48, 64, bad, DELTA, None) == 1
    assert "stride" in lib.gs_last_error().decode()
    tapes = (C.c_void_p * 1)(0x800004)
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(_seq().base), tapes, 1, 48, 64, prm, DELTA, None) == 1
    assert "tape" in lib.gs_last_error().decode()
    bseq = (_C.PicpBackwardSeq * 1)()
    assert lib.gs_projective_icp_robust_backward_batch_f32(bseq, 1, 48, 64, prm, DELTA, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_robust_backward_batch_f32")
    assert lib.gs_projective_icp_color_robust_batch_f32(C.pointer(_seq(color=0)), 1, 48, 64, prm, 0.1, DELTA, 0.0, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_color_robust_batch_f32")
    assert lib.gs_projective_icp_color_robust_batch_f32(C.pointer(_seq()), 1, 48, 64, prm, -1.0, DELTA, 0.0, None) == 1
    assert "color_weight" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_robust_rows_f32(C.pointer(_seq().base), 48, 64, 0, 0.1, 0.866, DELTA, *([None] * 7),
                                                 None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_robust_rows_f32")
    assert lib.gs_projective_icp_color_robust_rows_f32(C.pointer(_seq(model_intensity=0xD00004)), 48, 64, 4, 0.1, 0.866,
                                                       0.1, DELTA, 0.0, *([None] * 12), None) == 1
    assert "aligned" in lib.gs_last_error().decode()


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(color=False):
    H, W = 4, 5
    a = [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
         torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]
    return a + [torch.zeros(H, W, 3), torch.zeros(H, W, 4)] if color else a


def test_ops_check_the_thresholds():
    from gradslam_amd import ops
    plain = (ops.projective_icp, ops.projective_icp_rows)
    joint = (ops.projective_icp_color, ops.projective_icp_color_rows)
    for fns, color, kw, names in ((plain, False, {}, ("huber_delta",)),
                                  (joint, True, dict(color_weight=0.1), ("huber_delta", "color_huber_delta"))):
        for fn in fns:
            for name in names:
                for bad in (float("nan"), -1e-3, float("inf")):
                    with pytest.raises(ValueError, match=name):
                        fn(*_cpu_args(color), **kw, **{name: bad})
                for bad in ("0.1", True, None):
                    with pytest.raises(TypeError, match=name):
                        fn(*_cpu_args(color), **kw, **{name: bad})
                with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):      # a good value goes on to the call
                    fn(*_cpu_args(color), **kw, **{name: 0.005})
    for fn, color, kw in ((ops.projective_icp_rows, False, {}), (ops.projective_icp_color_rows, True, dict(color_weight=0.1))):
        with pytest.raises(TypeError, match="return_weights"):
            fn(*_cpu_args(color), **kw, return_weights=1)
    # the differentiable solve takes the threshold; the colour solve keeps refusing the switch
    with pytest.raises(ValueError, match="huber_delta"):
        ops.projective_icp(*_cpu_args(), differentiable=True, huber_delta=-1.0)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp(*_cpu_args(), differentiable=True, huber_delta=0.005)
    with pytest.raises(ValueError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(True), color_weight=0.1, huber_delta=0.005, differentiable=True)
    a = _cpu_args()
    tapes = torch.zeros(1, 328 * 10, dtype=torch.uint8)
    with pytest.raises(ValueError, match="huber_delta"):
        ops.projective_icp_backward_batch(a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None],
                                          [(a[6], a[7], None, None)], tapes, a[8][None], huber_delta=float("nan"))


def test_provider_and_drivers_check_and_carry_the_thresholds():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam import ICPSLAM, PointFusion
    prov = ProjectiveICPOdometryProvider(huber_delta=0.005, color_weight=0.2, color_huber_delta=0.02)
    assert (prov.huber_delta, prov.color_huber_delta, prov.color_weight) == (0.005, 0.02, 0.2)
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)   # five keys
    off = ProjectiveICPOdometryProvider()
    assert off.huber_delta == 0.0 and off.color_huber_delta == 0.0
    for name in ("huber_delta", "color_huber_delta"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                ProjectiveICPOdometryProvider(color_weight=0.2, **{name: bad})
        for bad in ("1", True, None):
            with pytest.raises(TypeError, match=name):
                ProjectiveICPOdometryProvider(color_weight=0.2, **{name: bad})
    with pytest.raises(ValueError, match="color_weight"):
        ProjectiveICPOdometryProvider(color_huber_delta=0.02)                     # no colour term to apply it to
    assert ProjectiveICPOdometryProvider(huber_delta=0.005, differentiable=True).differentiable
    with pytest.raises(ValueError, match="differentiable"):                       # this refusal stays
        ProjectiveICPOdometryProvider(color_weight=0.1, huber_delta=0.005, differentiable=True)
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, huber_delta=0.005, color_weight=0.2, color_huber_delta=0.02)
        assert (s.huber_delta, s.color_huber_delta) == (0.005, 0.02)
        assert (s.odomprov.huber_delta, s.odomprov.color_huber_delta) == (0.005, 0.02)
        assert s.odomprov._kwargs() == dict(stride=2, numiters=20, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
        assert cls(odom="projicp").odomprov.huber_delta == 0.0
        d = cls(odom="projicp", huber_delta=0.005, odom_differentiable=True)
        assert d.odomprov.differentiable and d.odomprov.huber_delta == 0.005
        for odom in ("gt", "icp", "gradicp"):
            for name in ("huber_delta", "color_huber_delta"):
                with pytest.raises(ValueError, match=name):
                    cls(odom=odom, **{name: 0.01})
                assert getattr(cls(odom=odom, **{name: 0.0}), name) == 0.0
        with pytest.raises(ValueError, match="huber_delta"):
            cls(odom="projicp", huber_delta=-1)
        with pytest.raises(TypeError, match="huber_delta"):
            cls(odom="projicp", huber_delta="1")
        with pytest.raises(ValueError, match="color_weight"):
            cls(odom="projicp", color_huber_delta=0.02)
        with pytest.raises(ValueError, match="differentiable"):
            cls(odom="projicp", color_weight=0.1, huber_delta=0.005, odom_differentiable=True)
