"""CPU tests of the projective ICP's Huber threshold from the residuals' median: the NumPy restatement
(tests/picp_scale_ref.py) -- the selection rule against a sort, its fall-backs to the plain and the constant-threshold
restatements, its exact behaviour under a power-of-two change of units, what it is for (the moved block, no tuned
number), its float64 adjoint with frozen thresholds against central differences, the float32 yardsticks of
tests/picp_scale_backward_cases.py -- and, without a GPU, the exports, the argument checks of the C entry points (made
before any HIP call) and of the Python layers."""
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
from tests import picp_robust_ref as rr
from tests import picp_scale_backward_cases as sc
from tests import picp_scale_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
K = sr.K_HUBER
FD_BOUND = 1e-6     # what tests/test_picp_robust_cpu.py holds the constant-threshold adjoint to
# steps relative to the input's scale, as there (the weight delta / |b| is curved: the truncation error of a central
# difference falls with the square of the step, the best step counts).  The thresholds here shrink with the residuals
# (a third iteration clips at a tenth of a millimetre, against a step of 1e-8 x 100 m, the vertex the cases move out of
# the view), so the ladder goes on below 1e-8, down to where the rounding of float64 takes over
FD_STEPS = (1e-6, 3e-7, 1e-7, 3e-8, 1e-8, 3e-9, 1e-9, 3e-10)
NEW = ("gs_projective_icp_scaled_scratch_bytes", "gs_projective_icp_color_scaled_scratch_bytes",
       "gs_projective_icp_scaled_batch_f32", "gs_projective_icp_scaled_rows_f32",
       "gs_projective_icp_color_scaled_batch_f32", "gs_projective_icp_scaled_backward_batch_f32")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------ the selection rule
def _by_sort(b, used):
    v = np.sort(np.abs(np.asarray(b, F)[used]))
    return v[(v.size - 1) // 2]


def _multisets():
    rng = np.random.default_rng(5)
    yield "random", rng.standard_normal(1001).astype(F) * F(0.01)
    yield "random even", rng.standard_normal(1000).astype(F)
    yield "tied", rng.integers(-3, 4, 500).astype(F) * F(2.0 ** -10)
    yield "all equal", np.full(77, -0.125, F)
    yield "n = 1", np.array([-3e-3], F)
    yield "n = 2", np.array([4e-3, -1e-3], F)
    yield "low bits only", (np.float32(1.0).view(np.uint32) + rng.integers(0, 1024, 400).astype(np.uint32)).view(F)
    yield "top bits only", (2.0 ** rng.integers(-120, 120, 300)).astype(F)
    yield "denormals and zeros", np.concatenate([np.zeros(5, F), (rng.integers(1, 1 << 20, 6).astype(np.uint32)).view(F)])
    yield "with an infinity", np.array([1.0, np.inf, -2.0, 3.0], F)


def test_the_selection_is_the_lower_median_of_a_sort():
    for name, b in _multisets():
        used = np.ones(b.size, bool)
        med, n = sr.lower_median_abs(b, used)
        assert n == b.size and med.dtype == F and bits(med) == bits(_by_sort(b, used)), name
        assert med in np.abs(b), name                               # an element of the set, never an average
        # every rank, not only the median's, on a subset
        keys = np.abs(b[:40]).view(np.uint32)
        assert [int(sr.select(keys, r)) for r in range(keys.size)] == sorted(keys.tolist()), name
        # slots that are not used do not count
        mask = np.arange(b.size) % 3 != 1
        if mask.any():
            assert bits(sr.lower_median_abs(b, mask)[0]) == bits(_by_sort(b, mask)), name
    assert sr.lower_median_abs(np.array([1.0, 3.0], F), np.ones(2, bool))[0] == 1.0       # even count: the smaller one


def test_the_threshold_is_one_float32_product_and_a_floor():
    b = np.array([1e-3, -2e-3, 5e-3, 0.0, 7e-3], F)
    used = np.array([True, True, True, False, True])
    c = F(K) * F(1.4826)
    assert sr.constant(K) == c and sr.constant(K).dtype == F
    d = sr.scale(b, used, K)
    assert d.dtype == F and bits(d) == bits(c * F(2e-3))            # rank (4 - 1) // 2 = 1 of (1, 2, 5, 7) mm
    assert bits(sr.scale(b, used, K, 0.5)) == bits(F(0.5)) and bits(sr.scale(b, used, K, 1e-4)) == bits(d)
    none = np.zeros(5, bool)
    assert bits(sr.scale(b, none, K, 0.5)) == bits(F(0.0))          # no used slot: +0.0, whatever the floor
    assert bits(sr.scale(np.zeros(5, F), used, K)) == bits(F(0.0))  # a zero median: the weights are off
    assert bits(sr.scale(np.full(5, np.nan, F), used, K, 0.25)) == bits(F(0.25))      # a NaN product is not above the floor


# ------------------------------------------------------------------------------------------ fall-backs
@pytest.mark.parametrize("stride", [1, 4])
def test_a_zero_median_gives_the_plain_bits_and_a_high_floor_the_constant_threshold_bits(stride):
    fx = pr.convergence_fixture()
    # more than half of the used residuals zero: the median, the threshold and with them the weights are off
    r = pr.rows(*pr.args_of(fx), fx["T0"], stride=stride)
    used = r.code == 0
    b = np.where(np.arange(r.b.size) % 3 == 0, F(1e-3), F(0.0)).astype(F)
    assert used.sum() > 100 and bits(sr.scale(b, used, K)) == bits(F(0.0))
    assert np.array_equal(rr.slot_weights(b, sr.scale(b, used, K), used), used.astype(F))
    # delta_k == 0 in an iteration: that iteration is the plain one.  k so small that c * med underflows to 0
    tiny = 1e-45
    Tz, trz, dz = sr.solve(*pr.args_of(fx), fx["T0"], tiny, stride=stride, numiters=3)
    Tp, trp = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride, numiters=3)
    assert (dz == 0).all() and np.array_equal(bits(Tz), bits(Tp)) and np.array_equal(bits(trz), bits(trp))
    # a floor above every c * med: the constant-threshold solve, bit for bit
    mv = rr.moved_block(fx)
    free = sr.solve(*pr.args_of(mv), mv["T0"], K, stride=stride)[2]
    floor = 0.05
    assert floor > free.max()
    Tf, trf, df = sr.solve(*pr.args_of(mv), mv["T0"], K, floor, stride=stride)
    Tc, trc = rr.solve(*pr.args_of(mv), mv["T0"], floor, stride=stride)
    assert (df == F(floor)).all() and np.array_equal(bits(Tf), bits(Tc)) and np.array_equal(bits(trf), bits(trc))


# ------------------------------------------------------------------------------------------ a change of units
@pytest.mark.parametrize("stride", [1, 4])
def test_a_power_of_two_change_of_units_scales_the_threshold_and_keeps_the_weights(stride):
    """depth, vertices, map points, the translation of both poses and dist_thresh times 4: at the first linearisation
    every b, the median and the threshold are exactly 4 times what they were and the weights have the same bits.  A
    constant huber_delta does not have this property."""
    fx = rr.moved_block(pr.convergence_fixture())
    big = sr.scaled_by(fx, 4.0)
    r1 = sr.rows(*pr.args_of(fx), fx["T0"], K, stride=stride, dist_thresh=0.1)
    r4 = sr.rows(*pr.args_of(big), big["T0"], K, stride=stride, dist_thresh=0.4)
    assert np.array_equal(r1.code, r4.code) and np.array_equal(r1.row, r4.row) and (r1.code == 0).sum() > 100
    assert np.array_equal(bits(r4.b), bits(r1.b * F(4))) and bits(r4.delta) == bits(r1.delta * F(4))
    assert np.array_equal(bits(r4.weight), bits(r1.weight))
    used = r1.code == 0
    assert 10 < (r1.weight[used] < 1).sum() < used.sum() - 10
    c1 = rr.rows(*pr.args_of(fx), fx["T0"], 0.005, stride=stride, dist_thresh=0.1)
    c4 = rr.rows(*pr.args_of(big), big["T0"], 0.005, stride=stride, dist_thresh=0.4)
    assert np.array_equal(c1.code, c4.code) and not np.array_equal(c1.weight, c4.weight)


# ------------------------------------------------------------------------------------------ what the rule is for
SCENES = [("wave", True, 1), ("wave", True, 4), ("facets", True, 1), ("facets", True, 4), ("wave", False, 1)]


@pytest.mark.parametrize("scene,moved,stride", SCENES)
def test_no_tuned_number_beats_the_hand_picked_constant(scene, moved, stride):
    """60 x 80, frame 5 against frame 0's map, 10 iterations, k = 1.345, no floor; the moved block of
    picp_robust_ref.moved_block.  Translation error against the ground truth in mm, by the restatements:

        scene, stride        plain    huber_delta = 0.005    median rule    clipped share of used rows, per iteration
        wave moved, 1        18.680   4.779                  0.597          0.16 .. 0.23
        wave moved, 4        20.498   5.323                  1.524          0.16 .. 0.20
        facets moved, 1      11.720   2.326                  0.007          0.16 .. 0.34
        facets moved, 4      10.944   1.878                  0.013          0.18 .. 0.33
        wave clean, 1         0.092   0.078                  0.112          0.11 .. 0.26

    The threshold falls from 18.9 mm at iteration 0 to 0.52 mm at iteration 9 on "wave moved, 1" (facets: 15.9 mm to
    9 um).  Moved: err(median rule) < err(0.005) < err(plain).  Clean "wave": the rule costs less than a factor of two.
    Every scene, every iteration: the clipped share lies strictly between 0 and 0.5 (the median itself is not clipped)."""
    fx = pr.convergence_fixture(scene=scene)
    if moved:
        fx = rr.moved_block(fx)
    Tp, _ = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride)
    T5, _ = rr.solve(*pr.args_of(fx), fx["T0"], 0.005, stride=stride)
    a = sr.association(*pr.args_of(fx), fx["T0"], K, stride=stride)
    ep, e5, em = (rr.translation_error(T, fx["gt"]) for T in (Tp, T5, a.pose))
    share = a.clipped.sum(1) / a.used.sum(1)
    print("%s %s stride %d: plain %.3f mm, 0.005 %.3f mm, median rule %.3f mm; share %.2f .. %.2f; delta %.3g .. %.3g"
          % (scene, "moved" if moved else "clean", stride, 1e3 * ep, 1e3 * e5, 1e3 * em, share.min(), share.max(),
             a.deltas[0], a.deltas[-1]))
    assert np.isfinite(a.trace).all() and (a.deltas > 0).all()
    if moved:
        assert em < e5 < ep
    else:
        assert em < 2 * ep
    assert (share > 0).all() and (share < 0.5).all()
    assert a.deltas[-1] < 0.1 * a.deltas[0]                    # no constant fits both ends of one solve


def test_the_joint_restatement_uses_the_rule_for_the_geometric_threshold_only():
    fx = rr.moved_block(pcr.textured_fixture(scene="plane"))
    T, trace, deltas = sr.color_solve(*pcr.args_of(fx), fx["T0"], 0.2, K, 0.0, 0.02, stride=2, numiters=4)
    assert np.isfinite(trace).all() and (deltas > 0).all() and np.unique(deltas).size > 1
    # a floor above every threshold: the constant-threshold joint restatement
    Tf, trf, df = sr.color_solve(*pcr.args_of(fx), fx["T0"], 0.2, K, 0.05, 0.02, stride=2, numiters=4)
    Tc, trc = rr.color_solve(*pcr.args_of(fx), fx["T0"], 0.2, 0.05, 0.02, stride=2, numiters=4)
    assert (df == F(0.05)).all() and np.array_equal(bits(Tf), bits(Tc)) and np.array_equal(bits(trf), bits(trc))
    assert not np.array_equal(T, Tf)


# ------------------------------------------------------------------------------------------ adjoint vs finite differences
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_adjoint_against_central_differences(name):
    """<adjoint, d> against central differences of the float64 weighted forward with the SAME frozen thresholds, clip
    flags and association, along a random direction of each of the four inputs; the best step counts"""
    c = sc.build(name)
    fx = c.fx
    x = [c.v.astype(np.float64), fx["points"].astype(np.float64), fx["normals"].astype(np.float64),
         np.asarray(fx["T0"], np.float64)]
    Tb = c.T_bar.astype(np.float64)
    grads = sr.adjoint(*x[:3], c.assoc, x[3], Tb)
    assert (grads[3][3] == 0).all()
    rng = np.random.default_rng(3)
    worst = 0.0
    for i, what in enumerate(sc.OUTPUTS):
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
            f1, _ = sr.forward(*hi[:3], c.assoc, hi[3])
            f0, _ = sr.forward(*lo[:3], c.assoc, lo[3])
            fd = float(np.sum(Tb[:3] * (f1 - f0)[:3])) / (2 * h * scale)
            best = min(best, abs(fd - want) / abs(want))
        print("%s %s: <adjoint, d> = %.6g, best relative error %.2e" % (name, what, want, best))
        worst = max(worst, best)
    assert worst <= FD_BOUND, (name, worst)


def test_the_adjoint_reads_every_iterations_own_threshold():
    c = sc.build("conv_s4")
    P, N = c.fx["points"], c.fx["normals"]
    got = sr.adjoint(c.v, P, N, c.assoc, c.fx["T0"], c.T_bar, poses=c.assoc.poses)
    one = np.full_like(c.assoc.deltas, c.assoc.deltas[0])
    const = sr.adjoint(c.v, P, N, c.assoc, c.fx["T0"], c.T_bar, deltas=one, poses=c.assoc.poses)
    same = rr.adjoint(c.v, P, N, c.assoc, c.fx["T0"], c.T_bar, float(c.assoc.deltas[0]), poses=c.assoc.poses)
    assert bc.rel_err(got[0], const[0]) > 1e-2
    for a, b in zip(const, same):                              # with one threshold it is the constant-threshold adjoint
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ yardsticks and cases
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_committed_gap_is_current(name):
    """the float32 yardstick the GPU suite uses is what this machine measures, within DRIFT"""
    c = sc.build(name)
    assert sc.claims(c) == (name in sc.MIXED) or name not in sc.MIXED
    got, want = sc.gaps(name), sc.GAP[name]
    print(name, got, want)
    for out, g, w in zip(sc.OUTPUTS, got, want):
        assert w / bc.DRIFT <= g <= w * bc.DRIFT, (name, out, g, w)
        assert w < 1e-2                                        # a yardstick that still measures something


def test_cases_cover_what_the_kernel_can_get_wrong():
    assert set(sc.GAP) == set(sc.CASES) and set(sc.MIXED) <= set(sc.CASES) and len(sc.MIXED) >= 2
    chunks = {-(-sc.build(n).v.shape[0] // 256) for n in sc.CASES}
    assert {1, 2, 8, 19} <= chunks, chunks
    assert sc.build("edge_s1").v.shape[0] % 256 != 0 and sc.build("edge_s3").v.shape[0] == 234
    assert sc.build("stale_dc").device_count is not None
    assert all(sc.build(n).numiters >= 3 for n in sc.CASES)
    for n in sc.CASES:                                         # some iteration has both kinds; two thresholds differ
        a = sc.build(n).assoc
        assert any(a.clipped[k].any() and (a.used[k] & ~a.clipped[k]).any() for k in range(a.used.shape[0]))
        assert np.unique(a.deltas).size >= 2
    for n in sc.NO_INLIER:
        c = sc.build(n)
        assert not c.assoc.used.any() and not c.assoc.clipped.any() and (c.assoc.trace == 0).all()
        assert np.array_equal(bits(c.assoc.deltas), bits(np.zeros(3, F)))       # n == 0: +0.0
        ref = sc.reference(c)
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
    # the scratch: the plain / colour one, then the keys (nslots uint32) and the threshold, each aligned
    for h, w, s in ((60, 80, 1), (37, 53, 3), (480, 640, 4)):
        ns = -(-h // s) * -(-w // s)
        for plain, scaled in ((lib.gs_projective_icp_scratch_bytes, lib.gs_projective_icp_scaled_scratch_bytes),
                              (lib.gs_projective_icp_color_scratch_bytes, lib.gs_projective_icp_color_scaled_scratch_bytes)):
            assert scaled(h, w, s) >= plain(h, w, s) + 4 * ns + 4 and scaled(h, w, s) % 256 == 0
    assert lib.gs_projective_icp_scaled_scratch_bytes(0, 64, 1) == 0
    assert lib.gs_projective_icp_color_scaled_scratch_bytes(48, 64, 0) == 0


def _seq(**kw):
    from tests.test_picp_color_cpu import _seq as color_seq
    return color_seq(**kw)


def _prm():
    return _C.PicpParams(4, 10, 1e-8, 0.1, 0.866)


def _calls(lib, q, prm):
    return {
        "gs_projective_icp_scaled_batch_f32":
            lambda k, fl: lib.gs_projective_icp_scaled_batch_f32(C.pointer(q.base), None, None, 1, 48, 64, prm, k, fl, None),
        "gs_projective_icp_scaled_rows_f32":
            lambda k, fl: lib.gs_projective_icp_scaled_rows_f32(C.pointer(q.base), 48, 64, 4, 0.1, 0.866, k, fl,
                                                                *([None] * 8), None),
        "gs_projective_icp_color_scaled_batch_f32":
            lambda k, fl: lib.gs_projective_icp_color_scaled_batch_f32(C.pointer(q), None, 1, 48, 64, prm, 0.1, k, fl, 0.0,
                                                                       None),
    }


@pytest.mark.parametrize("bad", [float("nan"), -1e-3, float("inf"), -float("inf"), 0.0])
def test_entry_points_reject_a_bad_huber_k_before_any_hip_call(bad):
    lib = _C.lib()
    q, prm = _seq(), _prm()
    for name, call in _calls(lib, q, prm).items():
        assert call(bad, 0.0) == 1, name                          # GS_ERR_INVALID
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "huber_k" in msg, msg
        if bad != 0.0:                                            # (0 is a valid floor)
            assert call(1.345, bad) == 1, name
            msg = lib.gs_last_error().decode()
            assert msg.startswith(name) and "huber_floor" in msg, msg


def test_entry_points_keep_the_checks_of_their_plain_counterparts():
    lib = _C.lib()
    prm = _prm()
    name = "gs_projective_icp_scaled_batch_f32"
    assert lib.gs_projective_icp_scaled_batch_f32(None, None, None, 1, 48, 64, prm, K, 0.0, None) == 1
    assert lib.gs_projective_icp_scaled_batch_f32(C.pointer(_seq(vertex=0).base), None, None, 1, 48, 64, prm, K, 0.0, None) == 1
    assert lib.gs_last_error().decode().startswith(name) and "NULL" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_scaled_batch_f32(C.pointer(_seq().base), None, None, 1, 0, 64, prm, K, 0.0, None) == 1
    bad = _C.PicpParams(0, 10, 1e-8, 0.1, 0.866)
    assert lib.gs_projective_icp_scaled_batch_f32(C.pointer(_seq().base), None, None, 1, 48, 64, bad, K, 0.0, None) == 1
    assert "stride" in lib.gs_last_error().decode()
    tapes = (C.c_void_p * 1)(0x800004)
    assert lib.gs_projective_icp_scaled_batch_f32(C.pointer(_seq().base), tapes, None, 1, 48, 64, prm, K, 0.0, None) == 1
    assert "tape" in lib.gs_last_error().decode()
    deltas = (C.c_void_p * 1)(0)
    assert lib.gs_projective_icp_scaled_batch_f32(C.pointer(_seq().base), None, deltas, 1, 48, 64, prm, K, 0.0, None) == 1
    assert "deltas" in lib.gs_last_error().decode()
    bseq = (_C.PicpBackwardSeq * 1)()
    assert lib.gs_projective_icp_scaled_backward_batch_f32(bseq, 1, 48, 64, prm, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_scaled_backward_batch_f32")
    assert lib.gs_projective_icp_scaled_backward_batch_f32(bseq, 1, 48, 64, bad, None) == 1
    assert "stride" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_color_scaled_batch_f32(C.pointer(_seq(color=0)), None, 1, 48, 64, prm, 0.1, K, 0.0, 0.0,
                                                        None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_color_scaled_batch_f32")
    assert lib.gs_projective_icp_color_scaled_batch_f32(C.pointer(_seq()), None, 1, 48, 64, prm, -1.0, K, 0.0, 0.0, None) == 1
    assert "color_weight" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_color_scaled_batch_f32(C.pointer(_seq()), None, 1, 48, 64, prm, 0.1, K, 0.0, -1.0, None) == 1
    assert "color_huber_delta" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_scaled_rows_f32(C.pointer(_seq().base), 48, 64, 0, 0.1, 0.866, K, 0.0, *([None] * 8),
                                                 None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_scaled_rows_f32")


def test_the_constant_threshold_backward_keeps_rejecting_every_negative_threshold():
    """the taped mode of the backward is a flag of its own, not a value of huber_delta: -1 is refused like -1e-3"""
    lib = _C.lib()
    bseq = (_C.PicpBackwardSeq * 1)()
    for bad in (-1.0, -1e-3, -2.0, float("nan")):
        assert lib.gs_projective_icp_robust_backward_batch_f32(bseq, 1, 48, 64, _prm(), bad, None) == 1, bad
        msg = lib.gs_last_error().decode()
        assert msg.startswith("gs_projective_icp_robust_backward_batch_f32") and "huber_delta" in msg, msg


def test_scaled_entries_reject_a_scratch_that_is_not_16_byte_aligned():
    """the select block reads the key table, which lies behind the solve's scratch, four keys at a time"""
    lib = _C.lib()
    for name, call in _calls(lib, _seq(scratch=0xA00008), _prm()).items():
        assert call(K, 0.0) == 1, name
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "16-byte aligned" in msg, msg
    # the entries without the rule take such a scratch as they did
    q = _seq(scratch=0xA00008, vertex=0)
    assert lib.gs_projective_icp_robust_batch_f32(C.pointer(q.base), None, 1, 48, 64, _prm(), 0.005, None) == 1
    assert "aligned" not in lib.gs_last_error().decode()


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(color=False):
    H, W = 4, 5
    a = [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
         torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]
    return a + [torch.zeros(H, W, 3), torch.zeros(H, W, 4)] if color else a


def test_ops_check_huber_k():
    from gradslam_amd import ops
    for fn, color, kw in ((ops.projective_icp, False, {}), (ops.projective_icp_rows, False, {}),
                          (ops.projective_icp_color, True, dict(color_weight=0.1))):
        for bad in (float("nan"), -1e-3, float("inf")):
            with pytest.raises(ValueError, match="huber_k"):
                fn(*_cpu_args(color), **kw, huber_k=bad)
        for bad in ("1.345", True, None):
            with pytest.raises(TypeError, match="huber_k"):
                fn(*_cpu_args(color), **kw, huber_k=bad)
        for good in (1.345, 2, 0, 0.0):                                          # a good value goes on to the call
            with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
                fn(*_cpu_args(color), **kw, huber_k=good)
    for fn, color, kw in ((ops.projective_icp, False, {}), (ops.projective_icp_color, True, dict(color_weight=0.1))):
        with pytest.raises(TypeError, match="return_scale"):
            fn(*_cpu_args(color), **kw, return_scale=1)
    a = _cpu_args()
    b = [t[None] for t in a[:6]]
    with pytest.raises(ValueError, match="huber_k"):
        ops.projective_icp_batch(*b, [(a[6], a[7], None, None)], a[8][None], huber_k=-1.0)
    # the differentiable solve takes the rule; the colour solve keeps refusing the switch
    with pytest.raises(ValueError, match="huber_k"):
        ops.projective_icp(*_cpu_args(), differentiable=True, huber_k=-1.0)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp(*_cpu_args(), differentiable=True, huber_k=1.345)
    with pytest.raises(ValueError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(True), color_weight=0.1, huber_k=1.345, differentiable=True)
    tapes = torch.zeros(1, 328 * 10, dtype=torch.uint8)
    with pytest.raises(ValueError, match="huber_k"):
        ops.projective_icp_backward_batch(*b, [(a[6], a[7], None, None)], tapes, a[8][None], huber_k=float("nan"))
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_backward_batch(*b, [(a[6], a[7], None, None)], tapes, a[8][None], huber_k=1.345)


def test_provider_and_drivers_check_and_carry_huber_k():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam import ICPSLAM, PointFusion
    prov = ProjectiveICPOdometryProvider(huber_k=1.345, huber_delta=1e-4)
    assert (prov.huber_k, prov.huber_delta) == (1.345, 1e-4)
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)   # five keys
    assert ProjectiveICPOdometryProvider().huber_k == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="huber_k"):
            ProjectiveICPOdometryProvider(huber_k=bad)
    for bad in ("1", True, None):
        with pytest.raises(TypeError, match="huber_k"):
            ProjectiveICPOdometryProvider(huber_k=bad)
    assert ProjectiveICPOdometryProvider(huber_k=1.345, differentiable=True).differentiable
    assert ProjectiveICPOdometryProvider(huber_k=2, color_weight=0.2, color_huber_delta=0.02).huber_k == 2
    with pytest.raises(ValueError, match="differentiable"):                       # this refusal stays
        ProjectiveICPOdometryProvider(color_weight=0.1, huber_k=1.345, differentiable=True)
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, huber_k=1.345, huber_delta=1e-4)
        assert (s.huber_k, s.odomprov.huber_k, s.odomprov.huber_delta) == (1.345, 1.345, 1e-4)
        assert s.odomprov._kwargs() == dict(stride=2, numiters=20, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
        assert cls(odom="projicp").odomprov.huber_k == 0.0
        d = cls(odom="projicp", huber_k=1.345, odom_differentiable=True)
        assert d.odomprov.differentiable and d.odomprov.huber_k == 1.345
        for odom in ("gt", "icp", "gradicp"):
            with pytest.raises(ValueError, match="huber_k"):
                cls(odom=odom, huber_k=1.345)
            assert cls(odom=odom, huber_k=0.0).huber_k == 0.0
        with pytest.raises(ValueError, match="huber_k"):
            cls(odom="projicp", huber_k=-1)
        with pytest.raises(TypeError, match="huber_k"):
            cls(odom="projicp", huber_k="1")
        with pytest.raises(ValueError, match="differentiable"):
            cls(odom="projicp", color_weight=0.1, huber_k=1.345, odom_differentiable=True)
