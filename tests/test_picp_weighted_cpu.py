"""CPU tests of the projective ICP's per-pixel weights: the NumPy restatement (tests/picp_weighted_ref.py) -- its two bit
identities (weights of all ones are the unweighted solve, a weight of 0 is a depth of 0), what a mask is worth on the
moved-block scenes, its float64 adjoint (the gradient to the weights included) against central differences -- and,
without a GPU, the exports, the argument checks of the C entry points (made before any HIP call) and of the Python
layers, and the ready-made sensor model."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import picp_color_ref as pcr
from tests import picp_color_scale_ref as csr
from tests import picp_grad_ref as gr
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr
from tests import picp_weighted_ref as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1e-6     # what tests/test_picp_backward_cpu.py holds the plain adjoint to
FD_STEPS = (1e-4, 1e-5, 1e-6, 1e-7)
DELTA, COLOR_DELTA, WEIGHT, K_HUBER = 0.005, 0.02, 0.2, 1.345
NEW = ("gs_projective_icp_weighted_batch_f32", "gs_projective_icp_weighted_rows_f32",
       "gs_projective_icp_color_weighted_batch_f32", "gs_projective_icp_color_weighted_rows_f32",
       "gs_projective_icp_weighted_backward_scratch_bytes", "gs_projective_icp_weighted_backward_batch_f32")
# the thresholds of the geometric solve: plain, huber_delta, huber_k (with a floor)
GEO = {"plain": dict(), "delta": dict(huber_delta=DELTA), "k": dict(huber_k=K_HUBER, huber_delta=0.001)}
# ... and of the joint solve, both colour thresholds among them
JOINT = {"plain": dict(), "delta": dict(huber_delta=DELTA, color_huber_delta=COLOR_DELTA),
         "k": dict(huber_k=K_HUBER), "ck": dict(color_huber_k=K_HUBER, color_huber_delta=0.005),
         "both": dict(huber_k=K_HUBER, huber_delta=0.001, color_huber_k=K_HUBER)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def unweighted_geo(fx, kw, **more):
    """(pose, trace, thresholds) of the restatements this one is built on"""
    if kw.get("huber_k", 0) > 0:
        return sr.solve(*pr.args_of(fx), fx["T0"], kw["huber_k"], kw.get("huber_delta", 0.0), **more)
    T, trace = rr.solve(*pr.args_of(fx), fx["T0"], kw.get("huber_delta", 0.0), **more)
    return T, trace, np.full(trace.shape[0], kw.get("huber_delta", 0.0), np.float32)


# ------------------------------------------------------------------------------------------ the rule
def test_which_weights_mask():
    w = np.array([1.0, 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-40, 2.0 ** -20, 2.0 ** 20, 3.4e38], np.float32)
    assert np.array_equal(wr.masks(w), [False, True, True, True, True, True, True, False, False, False, False])
    sp = wr.special_weights((17, 31))
    assert wr.masks(sp).any() and not wr.masks(sp).all() and np.isnan(sp).any() and np.isinf(sp).any()
    assert ((sp > 0) & (sp < np.finfo(np.float32).tiny)).any()            # a denormal, which does not mask


def test_total_weight_is_one_float32_product_and_masked_slots_are_code_6():
    fx = rr.moved_block(pr.convergence_fixture())
    w = wr.random_weights((60, 80), patch=(slice(0, 9), slice(0, 80)))
    r = wr.rows(*pr.args_of(fx), w, fx["T0"], DELTA)
    plain = rr.rows(*pr.args_of(fx), fx["T0"], DELTA)
    lat = wr.lattice(w, 1)
    used = r.code == 0
    m = r.code == wr.MASKED
    assert m.any() and (plain.code[m] != 1).all() and (lat[m] == 0).all() and (r.row[m] == -1).all()
    assert (r.a[m] == 0).all() and (r.b[m] == 0).all() and (r.weight[~used] == 0).all()
    assert np.array_equal(r.code[~m], plain.code[~m]) and np.array_equal(r.b[used], plain.b[used])
    assert same(r.weight[used], (lat[used] * plain.weight[used]).astype(np.float32))
    assert r.count == int(used.sum()) < plain.count
    t = rr.terms(r.code, r.a, r.b, r.weight)
    k = int(np.nonzero(used)[0][5])
    assert t[k, 27] == float(r.weight[k]) * (float(r.b[k]) * float(r.b[k]))
    # the median of the scaled solve leaves the masked slots out: it is the median of the slots that are used
    rk = wr.rows(*pr.args_of(fx), w, fx["T0"], 0.0, K_HUBER)
    assert rk.delta == sr.scale(plain.b, used, K_HUBER) != sr.scale(plain.b, plain.code == 0, K_HUBER)


# ------------------------------------------------------------------------------------------ identity 1: all ones
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("which", sorted(GEO))
def test_all_ones_is_the_unweighted_restatement_bit_for_bit(which, stride):
    fx = rr.moved_block(pr.convergence_fixture())
    ones = np.ones((60, 80), np.float32)
    want = unweighted_geo(fx, GEO[which], stride=stride, numiters=4)
    got = wr.solve(*pr.args_of(fx), ones, fx["T0"], stride=stride, numiters=4, **GEO[which])
    none = wr.solve(*pr.args_of(fx), None, fx["T0"], stride=stride, numiters=4, **GEO[which])
    for g, n, w in zip(got, none, want):
        assert same(g, w) and same(n, w)


@pytest.mark.parametrize("which", sorted(JOINT))
def test_all_ones_is_the_unweighted_joint_restatement_bit_for_bit(which):
    fx = rr.moved_block(pcr.textured_fixture(scene="plane"))
    kw = JOINT[which]
    want = csr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, kw.get("huber_k", 0.0), kw.get("huber_delta", 0.0),
                           kw.get("color_huber_k", 0.0), kw.get("color_huber_delta", 0.0), stride=2, numiters=3)
    got = wr.color_solve(*pcr.args_of(fx), np.ones((60, 80), np.float32), fx["T0"], WEIGHT, stride=2, numiters=3, **kw)
    for g, w in zip(got, want):
        assert same(g, w)
    assert (want[1][:, 8] > 50).all()


# ------------------------------------------------------------------------------------------ identity 2: mask = no depth
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("which", sorted(GEO))
def test_a_mask_is_a_zeroed_depth_with_the_frame_maps_kept(which, stride):
    fx = rr.moved_block(pr.convergence_fixture())
    w = wr.block_mask((60, 80))
    zfx = wr.zeroed_depth(fx, w)
    assert np.array_equal(zfx["vertex"], fx["vertex"]) and (zfx["depth"][rr.BLOCK] == 0).all()
    want = unweighted_geo(zfx, GEO[which], stride=stride, numiters=4)
    got = wr.solve(*pr.args_of(fx), w, fx["T0"], stride=stride, numiters=4, **GEO[which])
    for g, x in zip(got, want):
        assert same(g, x)
    r = wr.rows(*pr.args_of(fx), w, fx["T0"], stride=stride, **GEO[which])
    z = wr.rows(*pr.args_of(zfx), None, fx["T0"], stride=stride, **GEO[which])
    assert ((r.code != z.code) == ((r.code == wr.MASKED) & (z.code == 1))).all() and (r.code == wr.MASKED).any()
    for k in ("row", "a", "b", "sums", "weight"):
        assert same(np.asarray(getattr(r, k)), np.asarray(getattr(z, k))), k


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("which", sorted(JOINT))
def test_a_mask_is_a_zeroed_depth_in_the_joint_solve(which, stride):
    fx = rr.moved_block(pcr.textured_fixture(scene="plane"))
    w = wr.block_mask((60, 80))
    zfx = wr.zeroed_depth(fx, w)
    kw = JOINT[which]
    want = csr.color_solve(*pcr.args_of(zfx), fx["T0"], WEIGHT, kw.get("huber_k", 0.0), kw.get("huber_delta", 0.0),
                           kw.get("color_huber_k", 0.0), kw.get("color_huber_delta", 0.0), stride=stride, numiters=3)
    got = wr.color_solve(*pcr.args_of(fx), w, fx["T0"], WEIGHT, stride=stride, numiters=3, **kw)
    for g, x in zip(got, want):
        assert same(g, x)
    assert (want[1][:, 8] > 20).all()


# ------------------------------------------------------------------------------------------ what a mask is worth
TABLE = {}


def _table(scene, stride):
    """translation errors (metres) of the moved-block scene after 10 iterations: no weights, huber_delta 5 mm, huber_k
    1.345, the block masked"""
    key = (scene, stride)
    if key not in TABLE:
        fx = rr.moved_block(pr.convergence_fixture(scene=scene))
        err = lambda T: rr.translation_error(T, fx["gt"])   # noqa: E731
        none = wr.solve(*pr.args_of(fx), None, fx["T0"], stride=stride)[0]
        delta = wr.solve(*pr.args_of(fx), None, fx["T0"], DELTA, stride=stride)[0]
        k = wr.solve(*pr.args_of(fx), None, fx["T0"], 0.0, K_HUBER, stride=stride)[0]
        mask = wr.solve(*pr.args_of(fx), wr.block_mask((60, 80)), fx["T0"], stride=stride)[0]
        TABLE[key] = tuple(err(T) for T in (none, delta, k, mask))
    return TABLE[key]


@pytest.mark.parametrize("scene,stride,bound", [("wave", 1, 0.2e-3), ("wave", 4, 1e-3), ("facets", 1, 0.2e-3),
                                                ("facets", 4, None)])
def test_masking_the_moved_block(scene, stride, bound):
    """The 60 x 80 fixtures, frame 5 against frame 0's map, the block [15:38, 20:51] 4 cm nearer, 10 iterations;
    translation error against the ground truth by this restatement (mm):
        scene, stride      none     huber_delta 5 mm   huber_k 1.345   block masked
        wave moved, 1      18.680   4.779              0.597           0.135
        wave moved, 4      20.498   5.323              1.524           0.659
        facets moved, 1    11.720   2.326              0.007           0.073
        facets moved, 4    10.944   1.878              0.013           2.211"""
    none, delta, k, mask = _table(scene, stride)
    print("%s moved, stride %d: none %.3f mm, huber_delta %.3f, huber_k %.3f, masked %.3f"
          % (scene, stride, 1e3 * none, 1e3 * delta, 1e3 * k, 1e3 * mask))
    assert mask < none                       # every row: below its unweighted error
    if bound is not None:
        assert mask < bound


# ------------------------------------------------------------------------------------------ adjoint vs finite differences
CASES = {"s1_delta": (1, 4, dict(huber_delta=0.004)), "s4_plain": (4, 5, dict()), "s2_k": (2, 3, dict(huber_k=K_HUBER))}


def _case(name):
    stride, numiters, kw = CASES[name]
    fx = rr.moved_block(pr.convergence_fixture())
    w = wr.random_weights((60, 80), patch=(slice(8, 20), slice(30, 55)))
    assoc = wr.association(*pr.args_of(fx), w, fx["T0"], stride=stride, numiters=numiters, **kw)
    return fx, w, assoc, gr.lattice(fx["vertex"], stride), stride


@pytest.mark.parametrize("name", sorted(CASES))
def test_adjoint_against_central_differences(name):
    """<adjoint, d> against central differences of the float64 weighted forward (association, masks, clip flags and
    thresholds frozen) along a random direction of the weights, the vertices and the initial pose; the best step counts"""
    fx, w, assoc, v, stride = _case(name)
    assert (assoc.codes == wr.MASKED).any() and assoc.used.all(0).any() and (assoc.clipped.any() or name == "s4_plain")
    P, N = fx["points"].astype(np.float64), fx["normals"].astype(np.float64)
    x = {"w": assoc.wp.astype(np.float64), "v": v.astype(np.float64), "T0": np.asarray(fx["T0"], np.float64)}
    x["w"][wr.masks(assoc.wp)] = 0.0           # (never read: masked slots are not used)
    Tb = np.random.default_rng(31).standard_normal((4, 4))
    f = lambda y: wr.forward(y["v"], P, N, y["w"], assoc, y["T0"])[0]   # noqa: E731
    vb, _, _, T0b, wb = wr.adjoint(x["v"], P, N, x["w"], assoc, x["T0"], Tb)
    assert (wb[~assoc.used.any(0)] == 0).all() and np.abs(wb).max() > 0 and (T0b[3] == 0).all()
    rng = np.random.default_rng(3)
    worst = 0.0
    for key, grad in (("w", wb), ("v", vb), ("T0", T0b)):
        d = rng.standard_normal(x[key].shape)
        if key == "T0":
            d[3] = 0.0
        d[~np.isfinite(x[key])] = 0.0
        want = float(np.sum(grad * d))
        scale = float(np.nanmax(np.abs(x[key])))
        best = np.inf
        for h in FD_STEPS:
            hi, lo = dict(x), dict(x)
            hi[key], lo[key] = x[key] + h * scale * d, x[key] - h * scale * d
            fd = float(np.sum(Tb[:3] * (f(hi) - f(lo))[:3])) / (2 * h * scale)
            best = min(best, abs(fd - want) / abs(want))
        print("%s %s_bar: <adjoint, d> = %.6g, best relative error %.2e" % (name, key, want, best))
        worst = max(worst, best)
    assert worst <= FD_BOUND, (name, worst)


def test_the_adjoint_with_unit_weights_is_the_unweighted_one():
    fx = rr.moved_block(pr.convergence_fixture())
    assoc = wr.association(*pr.args_of(fx), None, fx["T0"], DELTA, stride=4, numiters=4)
    v = gr.lattice(fx["vertex"], 4)
    Tb = np.random.default_rng(31).standard_normal((4, 4))
    got = wr.adjoint(v, fx["points"], fx["normals"], assoc.wp, assoc, fx["T0"], Tb, poses=assoc.poses)
    ra = rr.association(*pr.args_of(fx), fx["T0"], DELTA, stride=4, numiters=4)
    want = rr.adjoint(v, fx["points"], fx["normals"], ra, fx["T0"], Tb, DELTA, poses=ra.poses)
    for g, x in zip(got[:4], want):
        assert np.abs(g - x).max() <= 1e-12 * np.abs(x).max()


# ------------------------------------------------------------------------------------------ the library
def test_new_symbols_are_declared_and_exported_at_abi_3():
    lib = _C.lib()
    assert set(NEW) <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays
    assert C.sizeof(_C.PicpSeq) == 136 and C.sizeof(_C.PicpBackwardSeq) == 168      # the layouts stay
    assert lib.gs_projective_icp_tape_bytes(1) == 328
    base = lib.gs_projective_icp_backward_scratch_bytes(48, 64, 4, 100)
    obase = lib.gs_projective_icp_ordered_backward_scratch_bytes(48, 64, 4, 100)
    slots = 12 * 16
    assert lib.gs_projective_icp_weighted_backward_scratch_bytes(48, 64, 4, 100, 0) == base + 256 * -(-slots * 8 // 256)
    assert lib.gs_projective_icp_weighted_backward_scratch_bytes(48, 64, 4, 100, 1) == obase + 256 * -(-slots * 8 // 256)
    assert lib.gs_projective_icp_weighted_backward_scratch_bytes(0, 64, 4, 100, 0) == 0


WEIGHTED_KERNELS = {
    "gs_picp.hip": {"gs_weighted_picp_linearize_kernel"},
    "gs_picp_color.hip": {"gs_weighted_picp_color_linearize_kernel"},
    "gs_picp_scale.hip": {"gs_weighted_picp_scale_keys_kernel", "gs_weighted_picp_scale_color_keys_kernel",
                          "gs_weighted_picp_scale_joint_keys_kernel"},
    "gs_picp_bwd.hip": {"gs_weighted_picp_bwd_point_kernel", "gs_ordered_weighted_picp_bwd_point_kernel"},
}


@pytest.mark.parametrize("src", sorted(WEIGHTED_KERNELS))
def test_weighted_kernels_use_no_scratch_and_spill_nothing(src):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), src, "gs_weighted_",
                        "gs_ordered_weighted_"], capture_output=True, text=True, cwd=REPO, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "weighted_" in ln and not ln.startswith("#")}
    assert set(rows) == WEIGHTED_KERNELS[src], r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        print(name, "VGPR", vgpr, "scratch", scratch, "occupancy", occ, "LDS", lds)
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
        # the forward kernels keep the 8 waves per SIMD of the instances they stand next to, the point stage its 4
        assert int(occ) >= (4 if "bwd" in name else 8), (name, occ)


def _seq(**kw):
    from tests.test_picp_color_cpu import _seq as color_seq
    return color_seq(**kw)


def _prm(**kw):
    from tests.test_picp_color_cpu import _prm as prm
    return prm(**kw)


def _bseq(**kw):
    """an ordered-backward descriptor that passes every check (fake pointers: nothing is dereferenced before a HIP call)"""
    q = _C.PicpOrderedBackwardSeq()
    names = ("vertex", "normal", "depth", "K16", "index", "model_pose16", "tape", "pose_bar16", "scratch")
    a = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}
    a.update(scratch_bytes=1 << 30)
    a.update(kw)
    for k, v in a.items():
        setattr(q.base, k, v)
    q.base.map = _C.MapView(0xA00000, 0xB00000, 0, 0, 100, 100, 0)
    return q


W1 = (C.c_void_p * 1)(0xE00000)


def _calls(lib):
    """every weighted entry as f(seq, bseq, prm, weights array, weights pointer, huber_delta, huber_k)"""
    return {
        "gs_projective_icp_weighted_batch_f32":
            lambda q, bq, prm, wa, wp, d, k: lib.gs_projective_icp_weighted_batch_f32(
                C.pointer(q.base), wa, None, None, 1, 48, 64, prm, d, k, None),
        "gs_projective_icp_weighted_rows_f32":
            lambda q, bq, prm, wa, wp, d, k: lib.gs_projective_icp_weighted_rows_f32(
                C.pointer(q.base), wp, 48, 64, prm.stride, 0.1, 0.866, d, k, *([None] * 8), None),
        "gs_projective_icp_color_weighted_batch_f32":
            lambda q, bq, prm, wa, wp, d, k: lib.gs_projective_icp_color_weighted_batch_f32(
                C.pointer(q), wa, None, None, 1, 48, 64, prm, 0.1, d, k, 0.0, 0.0, None),
        "gs_projective_icp_color_weighted_rows_f32":
            lambda q, bq, prm, wa, wp, d, k: lib.gs_projective_icp_color_weighted_rows_f32(
                C.pointer(q), wp, 48, 64, prm.stride, 0.1, 0.866, 0.1, d, k, 0.0, 0.0, *([None] * 14), None),
        "gs_projective_icp_weighted_backward_batch_f32":
            lambda q, bq, prm, wa, wp, d, k: lib.gs_projective_icp_weighted_backward_batch_f32(
                C.pointer(bq), wa, None, 1, 48, 64, prm, d, 0, 0, None, 0, None),
    }


def test_every_entry_refuses_a_bad_descriptor_before_any_hip_call():
    lib = _C.lib()
    for name, call in _calls(lib).items():
        backward = "backward" in name
        # the weights are announced by the entry: a NULL array (a NULL image for the rows entries) is refused
        assert call(_seq(), _bseq(), _prm(), None, None, 0.0, 0.0) == 1, name
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "weights" in msg, msg
        for bad in (float("nan"), -1e-3, float("inf")):
            assert call(_seq(), _bseq(), _prm(), W1, 0xE00000, bad, 0.0) == 1, name
            assert lib.gs_last_error().decode().startswith(name) and "huber_delta" in lib.gs_last_error().decode()
            if not backward:
                assert call(_seq(), _bseq(), _prm(), W1, 0xE00000, 0.0, bad) == 1, name
                assert "huber_k" in lib.gs_last_error().decode()
        # the checks of the unweighted counterparts
        assert call(_seq(vertex=0), _bseq(vertex=0), _prm(), W1, 0xE00000, 0.0, 0.0) == 1, name
        assert "NULL" in lib.gs_last_error().decode()
        assert call(_seq(), _bseq(), _prm(stride=0), W1, 0xE00000, 0.0, 0.0) == 1, name
        assert "stride" in lib.gs_last_error().decode()
        if backward:
            assert call(_seq(), _bseq(scratch_bytes=64), _prm(), W1, 0xE00000, 0.0, 0.0) == 1
            assert "scratch too small" in lib.gs_last_error().decode()
            assert call(_seq(), _bseq(tape=0x700004), _prm(), W1, 0xE00000, 0.0, 0.0) == 1
            assert "misaligned" in lib.gs_last_error().decode()
    # a scaled call checks its scratch's alignment, a taped one its tape, a colour one its model intensity
    q = _seq(scratch=0xA00008)
    assert lib.gs_projective_icp_weighted_batch_f32(C.pointer(q.base), W1, None, None, 1, 48, 64, _prm(), 0.0, 1.345,
                                                    None) == 1
    assert "16-byte aligned" in lib.gs_last_error().decode()
    tapes = (C.c_void_p * 1)(0x800004)
    assert lib.gs_projective_icp_weighted_batch_f32(C.pointer(_seq().base), W1, tapes, None, 1, 48, 64, _prm(), 0.0, 0.0,
                                                    None) == 1
    assert "tape" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_color_weighted_batch_f32(C.pointer(_seq(model_intensity=0xD00004)), W1, None, None, 1,
                                                          48, 64, _prm(), 0.1, 0.0, 0.0, 0.0, 0.0, None) == 1
    assert "aligned" in lib.gs_last_error().decode()
    assert lib.gs_projective_icp_color_weighted_batch_f32(C.pointer(_seq()), W1, None, None, 1, 48, 64, _prm(), -1.0,
                                                          0.0, 0.0, 0.0, 0.0, None) == 1
    assert "color_weight" in lib.gs_last_error().decode()
    # the ordered mode's own checks
    assert lib.gs_projective_icp_weighted_backward_batch_f32(C.pointer(_bseq(points_bar=0xF00000)), W1, None, 1, 48, 64,
                                                             _prm(), 0.0, 0, 1, None, 0, None) == 1
    assert "sort scratch" in lib.gs_last_error().decode()


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(color=False):
    H, W = 4, 5
    a = [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
         torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]
    return a + [torch.zeros(H, W, 3), torch.zeros(H, W, 4)] if color else a


def test_ops_check_the_weights():
    from gradslam_amd import ops
    good = torch.ones(4, 5)
    for fn, color, kw in ((ops.projective_icp, False, {}), (ops.projective_icp_rows, False, {}),
                          (ops.projective_icp_color, True, dict(color_weight=0.1)),
                          (ops.projective_icp_color_rows, True, dict(color_weight=0.1))):
        for bad in ("1", 1.0, np.ones((4, 5), np.float32)):
            with pytest.raises(TypeError, match="pixel_weights"):
                fn(*_cpu_args(color), **kw, pixel_weights=bad)
        with pytest.raises(TypeError, match="pixel_weights"):
            fn(*_cpu_args(color), **kw, pixel_weights=good.double())
        for bad in (torch.ones(5, 4), torch.ones(4, 5, 1), torch.ones(1, 4, 5)):
            with pytest.raises(ValueError, match="pixel_weights"):
                fn(*_cpu_args(color), **kw, pixel_weights=bad)
        with pytest.raises(ValueError, match="device"):
            fn(*_cpu_args(color), **kw, pixel_weights=good.to("meta"))
        with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):      # good weights go on to the call
            fn(*_cpu_args(color), **kw, pixel_weights=good)
    a = _cpu_args()
    batch = [a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None], [(a[6], a[7], None, None)], a[8][None]]
    with pytest.raises(ValueError, match="pixel_weights"):
        ops.projective_icp_batch(*batch, pixel_weights=torch.ones(2, 4, 5))
    with pytest.raises(ValueError, match="one pixel_weights entry per sequence"):
        ops.projective_icp_batch(*batch, pixel_weights=[good, None])
    with pytest.raises(ValueError, match="one .B, H, W. tensor"):
        ops.projective_icp_batch(*batch, pixel_weights=[good], differentiable=True)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_batch(*batch, pixel_weights=[None])
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp(*a, pixel_weights=good, differentiable=True, huber_k=1.345)
    # the colour solve keeps refusing the tape, with or without weights
    with pytest.raises(ValueError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(True), color_weight=0.1, differentiable=True, pixel_weights=good)
    with pytest.raises(ValueError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(True), color_weight=0.1, differentiable=True)
    tapes = torch.zeros(1, 328 * 10, dtype=torch.uint8)
    bw = batch[:7] + [tapes, a[8][None]]
    with pytest.raises(TypeError, match="want_pixel_weights"):
        ops.projective_icp_backward_batch(*bw, pixel_weights=good[None], want_pixel_weights=1)
    with pytest.raises(ValueError, match="want_pixel_weights"):
        ops.projective_icp_backward_batch(*bw, want_pixel_weights=True)
    with pytest.raises(ValueError, match="pixel_weights"):
        ops.projective_icp_backward_batch(*bw, pixel_weights=torch.ones(1, 5, 4))
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_backward_batch(*bw, pixel_weights=good[None], want_pixel_weights=True)
    assert ops.WeightedProjectiveICPFunction.forward.__code__.co_varnames[:9] == (
        "ctx", "vertex", "normal", "depth", "K", "index", "model_poses", "init_poses", "pixel_weights")
    assert ops.ProjectiveICPFunction.forward.__code__.co_varnames[:9] == (
        "ctx", "vertex", "normal", "depth", "K", "index", "model_poses", "init_poses", "cfg")       # its signature stays


def test_provider_and_drivers_check_and_carry_the_weights():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider, axial_noise_weights
    from gradslam_amd.slam import ICPSLAM, PointFusion
    f = lambda frames: None   # noqa: E731
    prov = ProjectiveICPOdometryProvider(pixel_weights=f, huber_k=1.345)
    assert prov.pixel_weights is f and ProjectiveICPOdometryProvider().pixel_weights is None
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)   # five keys
    for bad in (1.0, "mask", torch.ones(4, 5)):
        with pytest.raises(TypeError, match="pixel_weights"):
            ProjectiveICPOdometryProvider(pixel_weights=bad)
    assert ProjectiveICPOdometryProvider(pixel_weights=f, differentiable=True).differentiable
    assert ProjectiveICPOdometryProvider(pixel_weights=f, color_weight=0.2, color_huber_k=1.345).color_weight == 0.2
    with pytest.raises(ValueError, match="differentiable"):                       # this refusal stays
        ProjectiveICPOdometryProvider(pixel_weights=f, color_weight=0.1, differentiable=True)
    # what the callable returns is checked where it is used
    for ret, err in ((None, TypeError), (torch.ones(2, 5, 4), ValueError), (torch.ones(2, 4, 5).double(), TypeError)):
        p = ProjectiveICPOdometryProvider(pixel_weights=lambda frames, r=ret: r)
        with pytest.raises(err, match="pixel_weights"):
            p._weights(None, 2, 4, 5)
    p = ProjectiveICPOdometryProvider(pixel_weights=lambda frames: torch.ones(2, 1, 4, 5))
    assert tuple(p._weights(None, 2, 4, 5).shape) == (2, 4, 5)
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, odom_pixel_weights=f, huber_delta=0.005)
        assert s.odomprov.pixel_weights is f and cls(odom="projicp").odomprov.pixel_weights is None
        assert cls(odom="projicp", odom_pixel_weights=axial_noise_weights, odom_differentiable=True).odomprov.differentiable
        for odom in ("gt", "icp", "gradicp"):
            with pytest.raises(ValueError, match="odom_pixel_weights"):
                cls(odom=odom, odom_pixel_weights=f)
            cls(odom=odom, odom_pixel_weights=None)
        with pytest.raises(TypeError, match="odom_pixel_weights"):
            cls(odom="projicp", odom_pixel_weights=torch.ones(4, 5))
        with pytest.raises(ValueError, match="differentiable"):
            cls(odom="projicp", odom_pixel_weights=f, color_weight=0.1, odom_differentiable=True)


def test_axial_noise_weights_are_the_formula():
    from gradslam_amd.odometry import axial_noise_weights
    from gradslam_amd.structures.rgbdimages import RGBDImages
    rng = np.random.default_rng(5)
    z = rng.uniform(0.4, 4.0, (2, 1, 6, 7, 1)).astype(np.float32)
    z[0, 0, 2, 3, 0], z[1, 0, 0, 0, 0] = 0.0, 0.4
    depth = torch.from_numpy(z).requires_grad_(True)
    frames = RGBDImages(torch.zeros(2, 1, 6, 7, 3), depth, torch.eye(4).view(1, 1, 4, 4).repeat(2, 1, 1, 1))
    w = axial_noise_weights(frames)
    assert tuple(w.shape) == (2, 1, 6, 7) and w.dtype == torch.float32
    z64 = z[..., 0].astype(np.float64)
    want = np.where(z64 > 0, (0.0012 / (0.0012 + 0.0019 * (z64 - 0.4) ** 2)) ** 2, 0.0)
    assert np.abs(w.detach().numpy() - want).max() <= 4 * np.finfo(np.float32).eps       # a handful of float32 roundings of values <= 1
    assert w[0, 0, 2, 3] == 0 and w[1, 0, 0, 0] == 1 and (w.detach().numpy()[z[..., 0] > 0.4] < 1).all()
    w2 = axial_noise_weights(frames, sigma0=0.002, k=0.001, z0=1.0)
    want2 = np.where(z64 > 0, (0.002 / (0.002 + 0.001 * (z64 - 1.0) ** 2)) ** 2, 0.0)
    assert np.abs(w2.detach().numpy() - want2).max() <= 4 * np.finfo(np.float32).eps
    w.sum().backward()                                              # plain torch: differentiable in the depth
    assert depth.grad is not None and torch.isfinite(depth.grad).all() and depth.grad.abs().max() > 0
    doc = " ".join(axial_noise_weights.__doc__.split())
    assert "published Kinect v1 axial-noise constants" in doc and "not tuned here" in doc
    with pytest.raises(TypeError):
        axial_noise_weights(depth)
    with pytest.raises(ValueError, match="sigma0"):
        axial_noise_weights(frames, sigma0=0.0)
