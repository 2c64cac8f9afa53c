"""CPU tests of the projective ICP's backward pass: the float64 NumPy adjoint (tests/picp_grad_ref.py) against central
finite differences of its own forward, the float32 yardsticks of tests/picp_backward_cases.py, what the cases exercise,
the argument checks of the new C entry points and Python layers (made before any HIP call, so they run without a GPU),
the exported symbols and the register report of the backward kernels (cross-compiled)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_backward_cases as pc
from tests import picp_grad_ref as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1e-6     # relative to the directional derivative (float64 central differences are good to about 1e-10 here;
#                     the rest is headroom for the conditioning of ten chained 6x6 solves; a missing or mis-signed term
#                     shows at 1e-2 or worse)
FD_STEPS = (1e-4, 1e-5, 1e-6)


# ------------------------------------------------------------------------------------------ adjoint vs finite differences
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_adjoint_against_central_differences(name):
    """<adjoint, d> against (f(x + h d) - f(x - h d)) / 2h of the float64 forward along a random direction d of each of
    the four inputs, for a random upstream adjoint; the function is smooth but not linear, so the best of three steps
    (h x the input's scale) counts."""
    c = pc.build(name)
    fx = c.fx
    x = [c.v.astype(np.float64), fx["points"].astype(np.float64), fx["normals"].astype(np.float64),
         np.asarray(fx["T0"], np.float64)]
    Tb = c.T_bar.astype(np.float64)
    grads = gr.adjoint(*x[:3], c.assoc, x[3], Tb)
    assert (grads[3][3] == 0).all()
    rng = np.random.default_rng(3)
    worst = 0.0
    for i, what in enumerate(pc.OUTPUTS):
        d = rng.standard_normal(x[i].shape)
        if i == 3:
            d[3] = 0.0                                # (the bottom row of a pose is a constant)
        d[~np.isfinite(x[i])] = 0.0                   # (rows beyond the count hold NaN: they are never read)
        want = float(np.sum(grads[i] * d))
        scale = float(np.nanmax(np.abs(x[i])))
        best = np.inf
        for h in FD_STEPS:
            hi, lo = list(x), list(x)
            hi[i], lo[i] = x[i] + h * scale * d, x[i] - h * scale * d
            f1, _ = gr.forward(*hi[:3], c.assoc, hi[3])
            f0, _ = gr.forward(*lo[:3], c.assoc, lo[3])
            fd = float(np.sum(Tb[:3] * (f1 - f0)[:3])) / (2 * h * scale)
            best = min(best, abs(fd - want) / abs(want))
        print("%s %s: <adjoint, d> = %.6g, best relative error %.2e" % (name, what, want, best))
        worst = max(worst, best)
    print("%s: worst %.2e" % (name, worst))
    assert worst <= FD_BOUND, (name, worst)


def test_adjoint_at_the_taped_poses_is_close_to_the_chained_one():
    """evaluating every step at the float32 poses of the forward instead of the float64 chain's moves the adjoint by the
    float32 rounding of ten poses, not more"""
    c = pc.build("conv_s4")
    chained = gr.adjoint(c.v, c.fx["points"], c.fx["normals"], c.assoc, c.fx["T0"], c.T_bar)
    taped = gr.adjoint(c.v, c.fx["points"], c.fx["normals"], c.assoc, c.fx["T0"], c.T_bar, poses=c.assoc.poses)
    for a, b in zip(taped, chained):
        assert bc.rel_err(a, b) < 1e-3
    assert np.array_equal(c.assoc.poses[0], np.asarray(c.fx["T0"], np.float32))


# ------------------------------------------------------------------------------------------ yardsticks and cases
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_committed_gap_is_current(name):
    """the float32 yardstick the GPU suite uses is what this machine measures, within DRIFT"""
    c = pc.build(name)
    pc.claims(c)
    got, want = pc.gaps(name), pc.GAP[name]
    print(name, got, want)
    for out, g, w in zip(pc.OUTPUTS, got, want):
        assert w / bc.DRIFT <= g <= w * bc.DRIFT, (name, out, g, w)


def test_cases_cover_what_the_kernel_can_get_wrong():
    assert set(pc.GAP) == set(pc.CASES)
    assert {(v[1], v[2]) for v in pc.CASES.values()} >= {(1, 10), (4, 10), (4, 1), (3, 6), (1, 6)}
    # chunks: one partial chunk, 2 chunks, several chunks with a tail, 19 chunks
    chunks = {-(-pc.build(n).v.shape[0] // 256) for n in pc.CASES}
    assert {1, 2, 8, 19} <= chunks, chunks
    assert pc.build("edge_s1").v.shape[0] % 256 != 0
    assert sum(pc.build(n).device_count is not None for n in pc.CASES) >= 3
    for n in pc.NO_INLIER:
        c = pc.build(n)
        assert not c.assoc.used.any() and (c.assoc.trace == 0).all()
        ref = pc.reference(c)
        assert np.array_equal(ref[3][:3], c.T_bar[:3].astype(np.float64)) and (ref[3][3] == 0).all()
        assert all((r == 0).all() for r in ref[:3])


# ------------------------------------------------------------------------------------------ the library
def _lib():
    from gradslam_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from gradslam_amd.csrc import build
        build.build()
    return _C, _C.lib()


def test_new_symbols_are_declared_and_exported():
    _C, lib = _lib()
    names = {"gs_projective_icp_tape_bytes", "gs_projective_icp_tape_batch_f32",
             "gs_projective_icp_backward_scratch_bytes", "gs_projective_icp_backward_batch_f32"}
    assert names <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in names:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
    assert "typedef struct gs_picp_backward_seq" in header
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays
    assert lib.gs_projective_icp_tape_bytes(10) == 10 * 328 and lib.gs_projective_icp_tape_bytes(0) == 0
    # state + 12 float64 per chunk + 3 float64 per slot; the map buffers only when a map output is asked for
    small = lib.gs_projective_icp_backward_scratch_bytes(480, 640, 4, 0)
    assert 75 * 12 * 8 + 19200 * 24 <= small <= 75 * 12 * 8 + 19200 * 24 + 2048
    assert lib.gs_projective_icp_backward_scratch_bytes(480, 640, 4, 1_000_000) - small >= 2 * 24_000_000
    assert lib.gs_projective_icp_backward_scratch_bytes(480, 640, 0, 0) == 0
    assert lib.gs_projective_icp_backward_scratch_bytes(46341, 46341, 1, 0) == 0


def test_entry_points_check_their_arguments_before_any_hip_call():
    _C, lib = _lib()
    prm = _C.PicpParams(4, 10, 1e-8, 0.1, 0.8)
    one = C.c_void_p(256)           # (never dereferenced: every check comes before the first HIP call)
    seqs = (_C.PicpBackwardSeq * 1)()
    assert lib.gs_projective_icp_backward_batch_f32(None, 1, 48, 64, prm, None) == 1
    assert lib.gs_projective_icp_backward_batch_f32(seqs, 1, 48, 64, prm, None) == 1 and b"NULL" in lib.gs_last_error()
    u = seqs[0]
    for f in ("vertex", "normal", "depth", "K16", "index", "model_pose16", "tape", "pose_bar16", "scratch"):
        setattr(u, f, one)
    u.map = _C.MapView(one, one, 0, 0, 100, 100, 0)
    u.points_bar = one
    u.scratch_bytes = lib.gs_projective_icp_backward_scratch_bytes(48, 64, 4, 0)   # too small for a map output
    assert lib.gs_projective_icp_backward_batch_f32(seqs, 1, 48, 64, prm, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_backward_batch_f32") and \
        b"scratch too small" in lib.gs_last_error()
    u.tape = C.c_void_p(260)
    assert lib.gs_projective_icp_backward_batch_f32(seqs, 1, 48, 64, prm, None) == 1 and \
        b"misaligned" in lib.gs_last_error()
    bad = _C.PicpParams(0, 10, 1e-8, 0.1, 0.8)
    assert lib.gs_projective_icp_backward_batch_f32(seqs, 1, 48, 64, bad, None) == 1 and b"stride" in lib.gs_last_error()
    fseqs = (_C.PicpSeq * 1)()
    assert lib.gs_projective_icp_tape_batch_f32(fseqs, None, 1, 48, 64, prm, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_tape_batch_f32")
    tapes = (C.c_void_p * 1)(256)
    assert lib.gs_projective_icp_tape_batch_f32(fseqs, tapes, 1, 48, 64, prm, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_projective_icp_tape_batch_f32") and b"NULL" in lib.gs_last_error()


def test_backward_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp_bwd.hip",
                        "gs_picp_bwd_"], capture_output=True, text=True, cwd=REPO, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_picp_bwd_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_picp_bwd_scalar_kernel", "gs_picp_bwd_point_kernel", "gs_picp_bwd_cast_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        print(name, "VGPR", vgpr, "scratch", scratch, "occupancy", occ, "LDS", lds)
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
    # the point kernel: a block of 256 threads at 4 waves per SIMD or better
    assert int(rows["gs_picp_bwd_point_kernel"][0]) <= 128 and int(rows["gs_picp_bwd_point_kernel"][3]) >= 4


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(H=4, W=5):
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]


def test_ops_accept_and_type_check_the_switch():
    from gradslam_amd import ops
    assert issubclass(ops.ProjectiveICPFunction, torch.autograd.Function)
    assert callable(ops.projective_icp_backward_batch)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="differentiable"):
            ops.projective_icp(*_cpu_args(), differentiable=bad)
    a = _cpu_args()
    with pytest.raises(ValueError, match="out="):
        ops.projective_icp_batch(a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None],
                                 [(a[6], a[7], None, None)], a[8][None], differentiable=True,
                                 out=torch.zeros(1, 4, 4))
    with pytest.raises(_cpu_error()):            # there is no CPU path, with or without the switch
        ops.projective_icp(*_cpu_args(), differentiable=True)


def _cpu_error():
    from gradslam_amd import _C
    return _C.HipExtensionError


def test_provider_and_drivers_accept_and_type_check_the_switch():
    import gradslam_amd as gs
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    assert ProjectiveICPOdometryProvider().differentiable is False
    assert ProjectiveICPOdometryProvider(differentiable=True).differentiable is True
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="differentiable"):
            ProjectiveICPOdometryProvider(differentiable=bad)
    for cls in (gs.slam.ICPSLAM, gs.slam.PointFusion):
        assert cls(odom="projicp").odomprov.differentiable is False and cls(odom="projicp").odom_differentiable is False
        s = cls(odom="projicp", odom_differentiable=True, dsratio=2)
        assert s.odomprov.differentiable is True and s.odom_differentiable is True and s.odomprov.stride == 2
        for bad in (1, "yes", None):
            with pytest.raises(TypeError, match="odom_differentiable"):
                cls(odom="projicp", odom_differentiable=bad)
        with pytest.raises(ValueError, match="projicp"):
            cls(odom="gradicp", odom_differentiable=True)
        assert cls(odom="gradicp").odom_differentiable is False


def test_taped_map_updates_do_not_count_as_rewrites():
    """the guard of localize(differentiable=True) tells an in-place change of the buffers from a taped, out-of-place
    update: both bump _generation, only the first _rewrites()"""
    import gradslam_amd as gs
    pc_ = gs.Pointclouds(points=[torch.zeros(5, 3)], normals=[torch.zeros(5, 3)])
    g, r = pc_._generation, pc_._rewrites()
    pc_._invalidate()
    assert pc_._generation == g + 1 and pc_._rewrites() == r + 1
    pc_._invalidate()
    pc_._taped_swaps += 1
    assert pc_._generation == g + 2 and pc_._rewrites() == r + 1
