"""CPU tests of the projective-association ICP: the NumPy restatement (tests/picp_ref.py) against a plain float64
computation and math.fsum, its convergence on the synthetic sequence, the argument checks of the C entry points (made
before any HIP call, so they run without a GPU), the register report of the two kernels (cross-compiled) and the argument
checks of the Python layers."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import picp_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


def guess(fx):
    """a pose between the initial guess and the ground truth: every gate has slots on both sides"""
    T = np.array(fx["T0"], np.float32)
    T[:3, 3] = 0.5 * (fx["T0"][:3, 3] + fx["gt"][:3, 3])
    return T


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("stride", [1, 4])
def test_rows_agree_with_a_plain_float64_computation(stride):
    """Every float32 quantity of the per-slot stage is within a few roundings of its float64 value:
    s = T v: 3 products and 3 sums of magnitude <= |s|_max =: M (about 3 m), error <= 6 eps32 M;
    a[0:3] are copies; a[3:6] = n_i s_j - n_j s_i with |n| <= 1: 3 roundings of magnitude <= M plus 2 errors of s,
    <= (3 + 12) eps32 M; b = n . (p - s): three differences carrying the error of s (6 eps32 M each, |n_i| <= 1, their
    own roundings are of magnitude dist_th and below) and two sums, <= 3 * 6 eps32 M + 8 eps32 * 0.1 < 20 eps32 M.
    The codes agree wherever the float64 decision is not within 1e-4 (pixels / metres / cosine) of its boundary, three
    orders of magnitude above those roundings."""
    fx = pr.convergence_fixture()
    T = guess(fx)
    r = pr.rows(*pr.args_of(fx), T, stride=stride)
    H, W = fx["depth"].shape
    dist_th, dot_th = (float(x) for x in pr.thresholds())
    v = fx["vertex"][::stride, ::stride].reshape(-1, 3).astype(np.float64)
    n = fx["normal"][::stride, ::stride].reshape(-1, 3).astype(np.float64)
    d = fx["depth"][::stride, ::stride].reshape(-1)
    T64, M64, K = T.astype(np.float64), fx["model_pose"].astype(np.float64), fx["K"].astype(np.float64)
    s = v @ T64[:3, :3].T + T64[:3, 3]
    g = n @ T64[:3, :3].T
    q = (s - M64[:3, 3]) @ M64[:3, :3]
    z = np.where(d > 0, q[:, 2], 1.0)                 # (pixels without depth have no vertex: code 1 whatever follows)
    u = (K[0, 0] * q[:, 0] + K[0, 2] * z) / z
    w = (K[1, 1] * q[:, 1] + K[1, 2] * z) / z
    inside = (u > -1e-3) & (u < W - 0.999) & (w > -1e-3) & (w < H - 0.999) & (z > 0)
    hh = np.clip(np.rint(np.where(inside, w, 0)), 0, H - 1).astype(int)
    ww = np.clip(np.rint(np.where(inside, u, 0)), 0, W - 1).astype(int)
    row = np.where(inside, fx["index"][hh, ww], -1)
    ok = row >= 0
    p, m = fx["points"][np.where(ok, row, 0)].astype(np.float64), fx["normals"][np.where(ok, row, 0)].astype(np.float64)
    dist = np.linalg.norm(s - p, axis=1)
    dot = (g * m).sum(1)
    code = np.where(~(d > 0), 1, np.where(~inside, 2, np.where(~ok, 3, np.where(~(dist < dist_th), 4,
                                                                                  np.where(~(dot > dot_th), 5, 0)))))
    margin = 1e-4
    sure = (np.abs(u - np.floor(u) - 0.5) > margin) & (np.abs(w - np.floor(w) - 0.5) > margin) & \
        (np.abs(u + 1e-3) > margin) & (np.abs(u - (W - 0.999)) > margin) & (np.abs(w + 1e-3) > margin) & \
        (np.abs(w - (H - 0.999)) > margin) & (np.abs(dist - dist_th) > margin) & (np.abs(dot - dot_th) > margin)
    sure |= code == 1
    assert sure.mean() > 0.99
    assert np.array_equal(r.code[sure], code[sure])
    assert set(np.unique(r.code)) >= {0, 1, 3, 4} and r.count == (r.code == 0).sum() > 100
    used = (r.code == 0) & sure
    assert np.array_equal(r.row[used], row[used])
    M = np.abs(s[used]).max()
    a64 = np.concatenate([m, np.cross(s, m)], 1)      # s x n = (nz sy - ny sz, nx sz - nz sx, ny sx - nx sy)
    b64 = (m * (p - s)).sum(1)
    assert np.array_equal(r.a[used, :3], fx["normals"][row[used]])
    assert np.abs(r.a[used] - a64[used]).max() <= 15 * EPS32 * M
    assert np.abs(r.b[used] - b64[used]).max() <= 20 * EPS32 * M
    assert (r.a[r.code != 0] == 0).all() and (r.b[r.code != 0] == 0).all()
    assert (r.row[(r.code == 1) | (r.code == 2)] == -1).all()


@pytest.mark.parametrize("shape,stride", [((60, 80), 1), ((60, 80), 4), ((37, 53), 3), ((37, 53), 1)])
def test_reduction_equals_fsum_within_the_derived_bound(shape, stride):
    """a sum of n float64 terms in any order is within (n - 1) 2^-53 sum|term| of the exact sum (first order)"""
    fx = pr.convergence_fixture(*shape)
    r = pr.rows(*pr.args_of(fx), guess(fx), stride=stride)
    t = pr.terms(r.code, r.a, r.b)
    n = t.shape[0]
    assert n == math.prod(pr.lattice_shape(*shape, stride))
    for k in range(pr.NV):
        exact = math.fsum(t[:, k])
        bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(t[:, k]))
        assert abs(r.sums[k] - exact) <= bound, (k, r.sums[k], exact, bound)
    assert r.sums[27] > 0 and r.count > 0


def test_reduction_order_is_the_documented_tree():
    """256-slot chunks, adjacent pairs, chunks in ascending order: checked on terms whose sum depends on the order"""
    rng = np.random.default_rng(7)
    t = (rng.standard_normal((600, 3)) * 10.0 ** rng.integers(-8, 8, (600, 3))).astype(np.float64)
    S = pr.reduce_terms(t)
    x = np.zeros((768, 3))
    x[:600] = t
    part = []
    for c in range(3):
        y = x[256 * c:256 * (c + 1)]
        for _ in range(8):
            y = np.stack([y[2 * i] + y[2 * i + 1] for i in range(len(y) // 2)])
        part.append(y[0])
    assert np.array_equal(S, (part[0] + part[1]) + part[2])
    assert not np.array_equal(S, t.sum(0))      # (the order matters for these terms)


@pytest.mark.parametrize("stride", [1, 4])
def test_restatement_converges_on_the_wave_sequence(stride):
    """frame 5 against a map of frame 0, initial guess pose 0 (25 mm off), 10 iterations: within 1e-3 m of the ground
    truth with the project's own frame normals (measured: 9.2e-5 m at stride 1, 8.7e-4 m at stride 4)"""
    fx = pr.convergence_fixture()
    T, trace = pr.solve(*pr.args_of(fx), fx["T0"], stride=stride, numiters=10)
    start = np.linalg.norm(fx["T0"][:3, 3] - fx["gt"][:3, 3])
    err = np.linalg.norm(T[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    print("stride %d: translation error %.3g m (from %.3g m), inliers %s" % (stride, err, start, trace[:, 0]))
    assert 0.024 < start < 0.026
    assert err <= 1e-3
    assert trace[-1, 0] > 100 and np.isfinite(trace).all()
    assert np.abs(trace[-1, 2:]).max() < np.abs(trace[0, 2:]).max()


def test_six_frame_loop_stays_within_one_frame_of_motion():
    """restatement localisation + the oracle's fusion update over the 6 frames: the last pose is within 5 mm (one
    frame's motion) of the ground truth, where a constant-pose guess would be 25 mm off"""
    fx = pr.convergence_fixture()
    _, poses = pr.run_sequence(fx["seq"], stride=1, numiters=10)
    err = np.linalg.norm(poses[:, :3, 3].astype(np.float64) - fx["seq"]["poses"][:, :3, 3], axis=1)
    print("translation error per frame [m]:", err)
    assert err[-1] <= 5e-3


def test_no_inlier_keeps_the_pose_bits():
    fx = pr.convergence_fixture()
    a = pr.args_of(fx)
    a[pr.ARGS.index("index")] = np.full_like(fx["index"], -1)
    T0 = np.array(fx["T0"])
    T0[2, 0] = -0.0
    T, trace = pr.solve(*a, T0, numiters=3)
    assert np.array_equal(T.view(np.uint32), T0.view(np.uint32)) and (trace == 0).all()


# ------------------------------------------------------------------------------------------ the C entry points
def _seq(**kw):
    """a descriptor that passes every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and every
    case below is rejected before one)"""
    names = ("vertex", "normal", "depth", "K16", "index", "model_pose16", "init_pose16", "out_pose16", "trace", "scratch")
    a = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}
    a.update(points=0xA00000, normals=0xB00000, n_bound=100, n_dev=0)
    a.update(kw)
    q = _C.PicpSeq()
    for k in names:
        setattr(q, k, a[k])
    q.map = _C.MapView(a["points"], a["normals"], 0, 0, 100, a["n_bound"], a["n_dev"])
    return q


INVALID_SEQ = {
    "null_vertex": (dict(vertex=0), "NULL"),
    "null_normal": (dict(normal=0), "NULL"),
    "null_depth": (dict(depth=0), "NULL"),
    "null_K": (dict(K16=0), "NULL"),
    "null_index": (dict(index=0), "NULL"),
    "null_model_pose": (dict(model_pose16=0), "NULL"),
    "null_init_pose": (dict(init_pose16=0), "NULL"),
    "null_scratch": (dict(scratch=0), "NULL"),
    "null_points": (dict(points=0), "NULL"),
    "null_map_normals": (dict(normals=0), "NULL"),
    "negative_bound": (dict(n_bound=-1), "map size"),
}
INVALID_PRM = {
    "stride_zero": (dict(stride=0), "stride"),
    "no_iterations": (dict(numiters=0), "numiters"),
    "damp_zero": (dict(damp=0.0), "damp"),
    "damp_negative": (dict(damp=-1e-8), "damp"),
    "damp_nan": (dict(damp=float("nan")), "damp"),
    "dist_nan": (dict(dist_th=float("nan")), "NaN"),
    "dot_nan": (dict(dot_th=float("nan")), "NaN"),
}
INVALID_SIZE = {"no_rows": dict(H=0), "no_columns": dict(W=0), "negative": dict(H=-3), "too_large": dict(H=1 << 16, W=1 << 15)}


def _prm(**kw):
    a = dict(stride=4, numiters=10, damp=1e-8, dist_th=0.1, dot_th=0.866)
    a.update(kw)
    return _C.PicpParams(a["stride"], a["numiters"], a["damp"], a["dist_th"], a["dot_th"])


def _batch(lib, seq, prm, B=1, H=48, W=64):
    return lib.gs_projective_icp_batch_f32(seq, B, H, W, prm, None)


def _rows(lib, seq, H=48, W=64, stride=4, dist_th=0.1, dot_th=0.866):
    return lib.gs_projective_icp_rows_f32(seq, H, W, stride, dist_th, dot_th, None, None, None, None, None, None, None)


@pytest.mark.parametrize("case", sorted(INVALID_SEQ))
def test_entry_points_reject_a_bad_descriptor_before_any_hip_call(case):
    lib = _C.lib()
    change, word = INVALID_SEQ[case]
    for call, name in ((lambda q: _batch(lib, q, _prm()), "gs_projective_icp_batch_f32"),
                       (lambda q: _rows(lib, q), "gs_projective_icp_rows_f32")):
        assert call(C.pointer(_seq(**change))) == 1            # GS_ERR_INVALID
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and word in msg, msg


@pytest.mark.parametrize("case", sorted(INVALID_PRM))
def test_batch_entry_point_rejects_bad_parameters(case):
    lib = _C.lib()
    change, word = INVALID_PRM[case]
    assert _batch(lib, C.pointer(_seq()), _prm(**change)) == 1
    msg = lib.gs_last_error().decode()
    assert msg.startswith("gs_projective_icp_batch_f32") and word in msg, msg


@pytest.mark.parametrize("case", sorted(INVALID_SIZE))
def test_entry_points_reject_bad_sizes(case):
    lib = _C.lib()
    assert _batch(lib, C.pointer(_seq()), _prm(), **INVALID_SIZE[case]) == 1
    assert _rows(lib, C.pointer(_seq()), **INVALID_SIZE[case]) == 1
    size = dict(H=48, W=64)
    size.update(INVALID_SIZE[case])
    assert lib.gs_projective_icp_scratch_bytes(size["H"], size["W"], 4) == 0


def test_entry_points_reject_the_rest():
    lib = _C.lib()
    assert _batch(lib, None, _prm()) == 1 and _batch(lib, C.pointer(_seq()), None) == 1
    assert _batch(lib, C.pointer(_seq()), _prm(), B=0) == 1
    assert _batch(lib, C.pointer(_seq(out_pose16=0)), _prm()) == 1 and b"out_pose16" in lib.gs_last_error()
    assert _rows(lib, None) == 1 and _rows(lib, C.pointer(_seq()), stride=0) == 1
    assert _rows(lib, C.pointer(_seq()), dist_th=float("nan")) == 1
    assert lib.gs_projective_icp_scratch_bytes(48, 64, 0) == 0


def test_scratch_size_and_exports():
    lib = _C.lib()
    assert {"gs_projective_icp_batch_f32", "gs_projective_icp_rows_f32", "gs_projective_icp_scratch_bytes"} <= set(_C.EXPORTS)
    for (H, W, stride) in ((60, 80, 1), (37, 53, 3), (480, 640, 4), (1, 1, 1)):
        nchunks = -(-math.prod(pr.lattice_shape(H, W, stride)) // 256)
        assert lib.gs_projective_icp_scratch_bytes(H, W, stride) >= nchunks * (28 * 8 + 4)


def test_picp_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp.hip", "gs_picp_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_picp_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_picp_linearize_kernel", "gs_picp_finish_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
    assert int(rows["gs_picp_linearize_kernel"][0]) <= 64 and int(rows["gs_picp_linearize_kernel"][3]) >= 8
    assert int(rows["gs_picp_linearize_kernel"][6]) <= 2048


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(H=4, W=5):
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]


def test_ops_have_no_cpu_fallback():
    from gradslam_amd import ops
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp(*_cpu_args())
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_rows(*_cpu_args())
    a = _cpu_args()
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_batch(a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None],
                                 [(a[6], a[7], None, None, None, None)], a[8][None])


def test_ops_argument_errors():
    from gradslam_amd import ops
    for kw, word in ((dict(damp=0.0), "damp"), (dict(damp=-1.0), "damp"), (dict(numiters=0), "numiters"),
                     (dict(stride=0), "stride"), (dict(angle_thresh=-1), "angle_thresh"),
                     (dict(angle_thresh=90.5), "angle_thresh"), (dict(dist_thresh=float("nan")), "dist_thresh")):
        with pytest.raises(ValueError, match=word):
            ops.projective_icp(*_cpu_args(), **kw)
    for kw, word in ((dict(stride=2.0), "stride"), (dict(numiters=True), "numiters"), (dict(damp="1"), "damp")):
        with pytest.raises(TypeError, match=word):
            ops.projective_icp(*_cpu_args(), **kw)
    a = _cpu_args()
    a[0] = torch.zeros(4, 6, 3)
    with pytest.raises(ValueError, match="vertex"):
        ops.projective_icp(*a)
    a = _cpu_args()
    a[4] = a[4].to(torch.int32)
    with pytest.raises(ValueError, match="int64"):
        ops.projective_icp(*a)
    a = _cpu_args()
    a[6] = torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        ops.projective_icp(*a)
    a = _cpu_args()
    a[2] = torch.ones(5)
    with pytest.raises(ValueError, match="depth"):
        ops.projective_icp(*a)
    a = _cpu_args()
    a[5] = "pose"
    with pytest.raises(TypeError, match="model_pose"):
        ops.projective_icp(*a)


def test_provider_and_drivers():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam import ICPSLAM, PointFusion
    from gradslam_amd.structures.pointclouds import Pointclouds
    prov = ProjectiveICPOdometryProvider()
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
    with pytest.raises(TypeError, match="localize"):
        prov.provide(Pointclouds(), Pointclouds())
    with pytest.raises(TypeError, match="localize"):
        prov(Pointclouds(), Pointclouds())
    with pytest.raises(TypeError, match="live_frame"):
        prov.localize(Pointclouds(), "frame", torch.eye(4).view(1, 1, 4, 4))
    for kw in (dict(damp=0), dict(numiters=0), dict(stride=0), dict(angle_thresh=91)):
        with pytest.raises(ValueError):
            ProjectiveICPOdometryProvider(**kw)
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, numiters=7, damp=1e-6)
        assert type(s.odomprov) is ProjectiveICPOdometryProvider
        assert s.odomprov._kwargs() == dict(stride=2, numiters=7, damp=1e-6, dist_thresh=0.1, angle_thresh=30)
        assert cls(odom="projicp", dist_thresh=0.05).odomprov.dist_thresh == 0.05
        assert cls(odom="projicp").odomprov.stride == 4
        with pytest.raises(ValueError, match="projicp"):
            cls(odom="projective")
