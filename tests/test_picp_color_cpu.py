"""CPU tests of the projective ICP's colour term: the NumPy restatement (tests/picp_color_ref.py) against a plain float64
computation of the same rows, what the term is for (a textured plane, on which geometry alone slides), the argument checks
of the C entry points (made before any HIP call, so they run without a GPU), the exports, the register report of the new
kernels (cross-compiled) and the argument checks of the Python layers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import picp_color_ref as pc
from tests import picp_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
WEIGHT = 0.2


def guess(fx):
    T = np.array(fx["T0"], np.float32)
    T[:3, 3] = 0.5 * (fx["T0"][:3, 3] + fx["gt"][:3, 3])
    return T


# ------------------------------------------------------------------------------------------ the restatement
def test_model_intensity_of_the_fixture():
    fx = pc.textured_fixture(scene="wave")
    M, index = fx["model"], fx["index"]
    H, W = index.shape
    ok = M[..., 3] == 1
    assert set(np.unique(M[..., 3])) == {0.0, 1.0} and 0.5 < ok.mean() < 0.9
    assert not ok[0].any() and not ok[-1].any() and not ok[:, 0].any() and not ok[:, -1].any()
    assert (M[..., 1][~ok] == 0).all() and (M[..., 2][~ok] == 0).all()
    holes = np.argwhere(index < 0)
    assert len(holes) > 100
    for h, w in holes[:50]:      # a hole switches off itself and its four neighbours
        for dh, dw in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            if 0 <= h + dh < H and 0 <= w + dw < W:
                assert not ok[h + dh, w + dw]
    I64 = fx["view_color"].astype(np.float64) @ np.array([float(c) for c in pc.LUMA])
    assert np.abs(M[..., 0] - I64).max() <= 3 * EPS32          # three roundings of magnitude <= 1
    gx64 = 0.5 * (I64[1:-1, 2:] - I64[1:-1, :-2])
    inner = ok[1:-1, 1:-1]
    assert np.abs(M[1:-1, 1:-1, 1] - gx64)[inner].max() <= 4 * EPS32
    # the three channels differ: the luma weights matter
    assert np.abs(fx["view_color"][..., 0] - fx["view_color"][..., 1])[index >= 0].mean() > 0.05


@pytest.mark.parametrize("scene,stride", [("plane", 1), ("wave", 4)])
def test_colour_rows_agree_with_a_plain_float64_computation(scene, stride):
    """With eps = 2^-24 and every bound in terms of maxima of the float64 quantities themselves:
    model pixel: I carries 3 roundings of magnitude <= 1 (3 eps); gx, gy: a difference of two such values, halved
    exactly, one more rounding: |d gx| <= 3 eps + eps |gx| <= 4 eps.
    q = R_m^T (s - t_m) from s = T v: 6 roundings of magnitude <= M (|s|, |q| <= M, about 3 m) each: |d q| <= 12 eps M;
    u - w2, v - h2: u is a quotient of sums of magnitude <= U = fx M + cx zmax, 5 roundings plus the error of q through
    fx / z: |d u| <= 5 eps U / zmin + 12 eps M fx / zmin * 2 =: DU (about 1e-4 pixels); the difference is exact (Sterbenz
    does not apply in general, so one more eps of magnitude <= 1).
    r = Il - ((I + gx du) + gy dv): Il and I 3 eps each, the two products gx du, gy dv carry |d g| / 2 + G DU + eps G / 2
    each (|du|, |dv| <= 1/2, G = max |g|), three sums of magnitude <= 2: 6 eps.  Together
        |d r| <= 6 eps + 2 (2 eps + G DU + eps G) + 6 eps
    Jq: ax = gx fx: (4 eps + eps G) fx; the quotients by q2 and q2^2 add the relative error of q2 (12 eps M / zmin) and one
    rounding each; the third component has two products with q0, q1 (|q| <= M) and a sum.  With JM = G fx / zmin the
    size of Jq0, Jq1 and JM M / zmin that of Jq2, every component of Jq, and of Js = R_m Jq (5 more roundings, |R| <= 1),
    is within
        DJ = (4 eps fx / zmin) (1 + 2 M / zmin) + eps JM (1 + M / zmin) (2 + 24 M / zmin + 4 + 5) * 3
    (the factor 3: the three terms of a row of R_m).  The cross product s x Js: two products and a difference, each with
    the error of s (6 eps M) and of Js: <= 2 (M DJ + 6 eps M JS + eps M JS) + eps 2 M JS, JS = max |Js|.
    a_c, b_c: one more rounding and the factor w.  No bound is taken from the restatement's own output."""
    fx = pc.textured_fixture(scene=scene)
    T = guess(fx)
    r = pc.rows(*pc.args_of(fx), T, WEIGHT, stride=stride)
    assert r.color_count == r.colored.sum() > 100 and r.count > r.color_count      # ok = 0 pixels occur
    assert (r.code[r.colored] == 0).all()
    assert (r.ac[~r.colored] == 0).all() and (r.bc[~r.colored] == 0).all()
    H, W = fx["depth"].shape
    sel = r.colored
    v = fx["vertex"][::stride, ::stride].reshape(-1, 3).astype(np.float64)[sel]
    col = fx["color"][::stride, ::stride].reshape(-1, 3).astype(np.float64)[sel]
    T64, M64, K = T.astype(np.float64), fx["model_pose"].astype(np.float64), fx["K"].astype(np.float64)
    s = v @ T64[:3, :3].T + T64[:3, 3]
    q = (s - M64[:3, 3]) @ M64[:3, :3]
    u = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]
    w = K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
    h2, w2 = np.rint(w).astype(int), np.rint(u).astype(int)
    sure = (np.abs(u - np.floor(u) - 0.5) > 1e-3) & (np.abs(w - np.floor(w) - 0.5) > 1e-3)
    assert sure.mean() > 0.98
    luma64 = np.array([float(c) for c in pc.LUMA])
    I = fx["view_color"].astype(np.float64) @ luma64
    Ip = np.pad(I, 1)
    gx = (0.5 * (Ip[1:-1, 2:] - Ip[1:-1, :-2]))[h2, w2]
    gy = (0.5 * (Ip[2:, 1:-1] - Ip[:-2, 1:-1]))[h2, w2]
    assert (fx["model"][h2, w2, 3][sure] == 1).all()
    res = col @ luma64 - (I[h2, w2] + gx * (u - w2) + gy * (w - h2))
    Jq = np.stack([gx * K[0, 0] / q[:, 2], gy * K[1, 1] / q[:, 2],
                   -(gx * K[0, 0] * q[:, 0] + gy * K[1, 1] * q[:, 1]) / q[:, 2] ** 2], 1)
    Js = Jq @ M64[:3, :3].T
    a64 = WEIGHT * np.concatenate([Js, np.cross(s, Js)], 1)
    b64 = WEIGHT * res
    eps = EPS32
    Mx = max(np.abs(s).max(), np.abs(q).max())
    zmin, fxy = q[:, 2].min(), max(K[0, 0], K[1, 1])
    G = max(np.abs(gx).max(), np.abs(gy).max())
    U = fxy * Mx + max(K[0, 2], K[1, 2]) * q[:, 2].max()
    DU = 5 * eps * U / zmin + 24 * eps * Mx * fxy / zmin
    Dr = 6 * eps + 2 * (2 * eps + G * DU + eps * G) + 6 * eps
    JM = G * fxy / zmin
    JS = np.abs(Js).max()
    DJ = 3 * ((4 * eps * fxy / zmin) * (1 + 2 * Mx / zmin) + eps * JM * (1 + Mx / zmin) * (11 + 24 * Mx / zmin))
    DC = 2 * (Mx * DJ + 7 * eps * Mx * JS) + 2 * eps * Mx * JS
    wf = float(np.float32(WEIGHT))
    assert abs(wf - WEIGHT) <= eps * WEIGHT
    ea = np.abs(r.ac[sel] - a64)[sure]
    eb = np.abs(r.bc[sel] - b64)[sure]
    bound_j = wf * DJ + 2 * eps * wf * JS
    bound_c = wf * DC + 2 * eps * wf * Mx * JS * 2
    bound_b = wf * Dr + 2 * eps * wf * np.abs(res).max()
    print("%s stride %d: |d a_c[:3]| %.3g (bound %.3g), |d a_c[3:]| %.3g (bound %.3g), |d b_c| %.3g (bound %.3g)"
          % (scene, stride, ea[:, :3].max(), bound_j, ea[:, 3:].max(), bound_c, eb.max(), bound_b))
    assert ea[:, :3].max() <= bound_j
    assert ea[:, 3:].max() <= bound_c
    assert eb.max() <= bound_b
    assert np.abs(a64).max() > 1e3 * bound_c and np.abs(b64).max() > 1e3 * bound_b      # (the bounds say something)


def test_joint_terms_and_sums():
    """each term is the geometric product plus the colour product; weight 0 leaves the plain sums"""
    fx = pc.textured_fixture(scene="plane")
    T = guess(fx)
    r = pc.rows(*pc.args_of(fx), T, WEIGHT, stride=2)
    plain = pr.rows(*pr.args_of(fx), T, stride=2)
    assert np.array_equal(r.code, plain.code) and np.array_equal(r.a, plain.a) and r.count == plain.count
    t = pc.joint_terms(r.code, r.a, r.b, r.ac, r.bc)
    k = np.nonzero(r.colored)[0][7]
    assert t[k, 27] == float(r.b[k]) ** 2 + float(r.bc[k]) ** 2
    assert t[k, 1] == float(r.a[k, 0]) * float(r.a[k, 1]) + float(r.ac[k, 0]) * float(r.ac[k, 1])
    assert r.sums[27] > plain.sums[27] and not np.array_equal(r.sums, plain.sums)
    zero = pc.rows(*pc.args_of(fx), T, 0.0, stride=2)
    assert np.array_equal(zero.sums, plain.sums) and zero.color_count == r.color_count


# ------------------------------------------------------------------------------------------ what the term is for
def test_the_colour_term_pins_a_textured_plane_that_geometry_alone_slides_on():
    """"plane" (z = 2) at 60 x 80, frame 5 localised from pose 0 (25 mm off), 15 iterations, stride 1.
    The restatement's own numbers: color_weight 0: 47.6 mm (worse than the start); color_weight 0.2: 1.72 mm."""
    fx = pc.textured_fixture(scene="plane")
    start = np.linalg.norm(fx["T0"][:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    Tg, _ = pr.solve(*pr.args_of(fx), fx["T0"], stride=1, numiters=15)
    Tc, trace = pc.solve(*pc.args_of(fx), fx["T0"], WEIGHT, stride=1, numiters=15)
    eg = np.linalg.norm(Tg[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    ec = np.linalg.norm(Tc[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    print("plane: start %.4g m, geometry only %.4g m, colour weight %.2g %.4g m; colour rows %s"
          % (start, eg, WEIGHT, ec, trace[:, 8]))
    assert 0.024 < start < 0.026
    assert eg > start
    assert ec <= 0.1 * start
    assert trace.shape == (15, 9) and (trace[:, 8] > 100).all() and (trace[:, 8] < trace[:, 0]).all()


def test_the_colour_term_does_not_disturb_the_wave():
    """"wave": the joint solve stays within the plain test's 1e-3 m (the restatement's own number: 0.0885 mm at weight
    0.2, 0.0918 mm without)"""
    fx = pc.textured_fixture(scene="wave")
    Tc, trace = pc.solve(*pc.args_of(fx), fx["T0"], WEIGHT, stride=1, numiters=15)
    ec = np.linalg.norm(Tc[:3, 3].astype(np.float64) - fx["gt"][:3, 3])
    print("wave: colour weight %.2g: %.4g m" % (WEIGHT, ec))
    assert ec <= 1e-3 and np.isfinite(trace).all()


def test_six_frame_loop_on_the_plane_needs_the_colour_term():
    """restatement localisation (stride 2, 10 iterations) + the oracle's fusion update over the 6 textured "plane" frames:
    with color_weight 1.0 the last pose is within 5 mm (one frame's motion) of the ground truth, without the term it is
    not.  The restatement's own numbers: 3.26 mm with the weight, 47.7 mm without (and 4.55 mm at weight 0.2: from the
    second frame on the surfels no longer sit on the pixel centres of the view, which the model intensity takes them to
    do, and a larger weight only removes the pull of the geometric rows)."""
    seq = pc.textured_sequence(6, 60, 80, "plane")
    err = {}
    for w in (1.0, 0.0):
        poses = pc.run_sequence(seq, w, stride=2, numiters=10)
        err[w] = np.linalg.norm(poses[:, :3, 3].astype(np.float64) - seq["poses"][:, :3, 3], axis=1)
        print("plane, weight %.2g: translation error per frame [m]: %s" % (w, err[w]))
    assert err[1.0][-1] <= 5e-3 < err[0.0][-1]


def test_no_geometric_inlier_keeps_the_pose_bits():
    fx = pc.textured_fixture(scene="plane")
    a = pc.args_of(fx)
    a[pc.ARGS.index("index")] = np.full_like(fx["index"], -1)
    T0 = np.array(fx["T0"])
    T0[2, 0] = -0.0
    T, trace = pc.solve(*a, T0, WEIGHT, numiters=3)
    assert np.array_equal(T.view(np.uint32), T0.view(np.uint32)) and (trace == 0).all()


# ------------------------------------------------------------------------------------------ the C entry points
def _seq(**kw):
    """a descriptor that passes every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and every
    case below is rejected before one)"""
    names = ("vertex", "normal", "depth", "K16", "index", "model_pose16", "init_pose16", "out_pose16", "trace", "scratch")
    a = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}
    a.update(points=0xA00000, normals=0xB00000, n_bound=100, n_dev=0, color=0xC00000, model_intensity=0xD00000)
    a.update(kw)
    q = _C.PicpColorSeq()
    for k in names:
        setattr(q.base, k, a[k])
    q.base.map = _C.MapView(a["points"], a["normals"], 0, 0, 100, a["n_bound"], a["n_dev"])
    q.color, q.model_intensity = a["color"], a["model_intensity"]
    return q


def _prm(**kw):
    a = dict(stride=4, numiters=10, damp=1e-8, dist_th=0.1, dot_th=0.866)
    a.update(kw)
    return _C.PicpParams(a["stride"], a["numiters"], a["damp"], a["dist_th"], a["dot_th"])


def _batch(lib, seq, prm, B=1, H=48, W=64, weight=0.1):
    return lib.gs_projective_icp_color_batch_f32(seq, B, H, W, prm, weight, None)


def _rows(lib, seq, H=48, W=64, stride=4, dist_th=0.1, dot_th=0.866, weight=0.1):
    return lib.gs_projective_icp_color_rows_f32(seq, H, W, stride, dist_th, dot_th, weight, *([None] * 10), None)


INVALID_SEQ = {
    "null_vertex": (dict(vertex=0), "NULL"), "null_normal": (dict(normal=0), "NULL"),
    "null_depth": (dict(depth=0), "NULL"), "null_K": (dict(K16=0), "NULL"), "null_index": (dict(index=0), "NULL"),
    "null_model_pose": (dict(model_pose16=0), "NULL"), "null_init_pose": (dict(init_pose16=0), "NULL"),
    "null_scratch": (dict(scratch=0), "NULL"), "null_points": (dict(points=0), "NULL"),
    "null_map_normals": (dict(normals=0), "NULL"), "negative_bound": (dict(n_bound=-1), "map size"),
    "null_color": (dict(color=0), "NULL"), "null_model": (dict(model_intensity=0), "NULL"),
    "misaligned_model": (dict(model_intensity=0xD00004), "aligned"),
}


@pytest.mark.parametrize("case", sorted(INVALID_SEQ))
def test_entry_points_reject_a_bad_descriptor_before_any_hip_call(case):
    lib = _C.lib()
    change, word = INVALID_SEQ[case]
    for call, name in ((lambda q: _batch(lib, q, _prm()), "gs_projective_icp_color_batch_f32"),
                       (lambda q: _rows(lib, q), "gs_projective_icp_color_rows_f32")):
        assert call(C.pointer(_seq(**change))) == 1            # GS_ERR_INVALID
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and word in msg, msg


@pytest.mark.parametrize("weight", [float("nan"), -0.1, float("inf"), -float("inf")])
def test_entry_points_reject_a_bad_weight(weight):
    lib = _C.lib()
    for call, name in ((lambda: _batch(lib, C.pointer(_seq()), _prm(), weight=weight), "gs_projective_icp_color_batch_f32"),
                       (lambda: _rows(lib, C.pointer(_seq()), weight=weight), "gs_projective_icp_color_rows_f32")):
        assert call() == 1
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "color_weight" in msg, msg


@pytest.mark.parametrize("change,word", [(dict(stride=0), "stride"), (dict(numiters=0), "numiters"),
                                         (dict(damp=0.0), "damp"), (dict(damp=float("nan")), "damp"),
                                         (dict(dist_th=float("nan")), "NaN"), (dict(dot_th=float("nan")), "NaN")])
def test_batch_entry_point_rejects_bad_parameters(change, word):
    lib = _C.lib()
    assert _batch(lib, C.pointer(_seq()), _prm(**change)) == 1
    msg = lib.gs_last_error().decode()
    assert msg.startswith("gs_projective_icp_color_batch_f32") and word in msg, msg


@pytest.mark.parametrize("size", [dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 16, W=1 << 15)])
def test_entry_points_reject_bad_sizes(size):
    lib = _C.lib()
    assert _batch(lib, C.pointer(_seq()), _prm(), **size) == 1
    assert _rows(lib, C.pointer(_seq()), **size) == 1
    full = dict(H=48, W=64)
    full.update(size)
    assert lib.gs_projective_icp_color_scratch_bytes(full["H"], full["W"], 4) == 0
    assert lib.gs_model_intensity_f32(0x100000, 0x200000, 1, full["H"], full["W"], 0x300000, None) == 1
    assert lib.gs_last_error().decode().startswith("gs_model_intensity_f32")


def test_entry_points_reject_the_rest():
    lib = _C.lib()
    assert _batch(lib, None, _prm()) == 1 and _batch(lib, C.pointer(_seq()), None) == 1
    assert _batch(lib, C.pointer(_seq()), _prm(), B=0) == 1
    assert _batch(lib, C.pointer(_seq(out_pose16=0)), _prm()) == 1 and b"out_pose16" in lib.gs_last_error()
    assert _rows(lib, None) == 1 and _rows(lib, C.pointer(_seq()), stride=0) == 1
    assert _rows(lib, C.pointer(_seq()), dist_th=float("nan")) == 1
    assert lib.gs_projective_icp_color_scratch_bytes(48, 64, 0) == 0
    mi = lib.gs_model_intensity_f32
    for args, word in (((0, 0x200000, 1, 48, 64, 0x300000), "NULL"), ((0x100000, 0, 1, 48, 64, 0x300000), "NULL"),
                       ((0x100000, 0x200000, 1, 48, 64, 0), "NULL"), ((0x100000, 0x200000, 0, 48, 64, 0x300000), "sizes"),
                       ((0x100000, 0x200000, 1, 48, 64, 0x300004), "aligned"),
                       ((0x100000, 0x200000, 1, 48, 64, 0x100000), "input")):
        assert mi(*args, None) == 1
        msg = lib.gs_last_error().decode()
        assert msg.startswith("gs_model_intensity_f32") and word in msg, msg


def test_exports_abi_and_scratch_size():
    lib = _C.lib()
    names = {"gs_model_intensity_f32", "gs_projective_icp_color_batch_f32", "gs_projective_icp_color_rows_f32",
             "gs_projective_icp_color_scratch_bytes"}
    assert names <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in names:
        assert "GS_API" in header and n + "(" in header, n
    assert "typedef struct gs_picp_color_seq" in header
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays
    assert C.sizeof(_C.PicpColorSeq) == C.sizeof(_C.PicpSeq) + 16
    for (H, W, stride) in ((60, 80, 1), (37, 53, 3), (480, 640, 4), (1, 1, 1)):
        nchunks = -(-np.prod(pr.lattice_shape(H, W, stride)) // 256)
        assert lib.gs_projective_icp_color_scratch_bytes(H, W, stride) >= nchunks * (28 * 8 + 4 + 4)
        assert lib.gs_projective_icp_color_scratch_bytes(H, W, stride) > lib.gs_projective_icp_scratch_bytes(H, W, stride)


def test_colour_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp_color.hip",
                        "gs_picp_color_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_picp_color_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_picp_color_intensity_kernel", "gs_picp_color_linearize_kernel",
                         "gs_picp_color_finish_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
    # as the plain linearise kernel: 8 waves per SIMD (<= 64 VGPRs), the reduction's LDS only
    assert int(rows["gs_picp_color_linearize_kernel"][0]) <= 64 and int(rows["gs_picp_color_linearize_kernel"][3]) >= 8
    assert int(rows["gs_picp_color_linearize_kernel"][6]) <= 2048


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(H=4, W=5):
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4),
            torch.zeros(H, W, 3), torch.zeros(H, W, 4)]


def test_ops_have_no_cpu_fallback():
    from gradslam_amd import ops
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_color(*_cpu_args(), color_weight=0.1)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_color_rows(*_cpu_args(), color_weight=0.1)
    a = _cpu_args()
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_color_batch(a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None],
                                       [(a[6], a[7], None, None, None, None)], a[8][None], a[9][None], a[10][None],
                                       color_weight=0.1)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.model_intensity(torch.zeros(4, 5, 3), torch.zeros(4, 5, dtype=torch.int64))


def test_ops_argument_errors():
    from gradslam_amd import ops
    for fn in (ops.projective_icp_color, ops.projective_icp_color_rows):
        for bad in (float("nan"), -1e-3, float("inf")):
            with pytest.raises(ValueError, match="color_weight"):
                fn(*_cpu_args(), color_weight=bad)
        for bad in ("0.1", True, None):
            with pytest.raises(TypeError, match="color_weight"):
                fn(*_cpu_args(), color_weight=bad)
        with pytest.raises(TypeError):
            fn(*_cpu_args())                           # the weight has no default here
    with pytest.raises(ValueError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(), color_weight=0.1, differentiable=True)
    with pytest.raises(TypeError, match="differentiable"):
        ops.projective_icp_color(*_cpu_args(), color_weight=0.1, differentiable=1)
    for kw, word in ((dict(damp=0.0), "damp"), (dict(numiters=0), "numiters"), (dict(stride=0), "stride"),
                     (dict(angle_thresh=90.5), "angle_thresh"), (dict(dist_thresh=float("nan")), "dist_thresh")):
        with pytest.raises(ValueError, match=word):
            ops.projective_icp_color(*_cpu_args(), color_weight=0.1, **kw)
    a = _cpu_args()
    a[0] = torch.zeros(4, 6, 3)
    with pytest.raises(ValueError, match="vertex"):
        ops.projective_icp_color(*a, color_weight=0.1)
    a = _cpu_args()
    a[9] = "colour"
    with pytest.raises(TypeError, match="color"):
        ops.projective_icp_color(*a, color_weight=0.1)
    with pytest.raises(ValueError, match="index"):
        ops.model_intensity(torch.zeros(4, 5, 3), torch.zeros(4, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        ops.model_intensity(torch.zeros(4, 5, 3), torch.zeros(4, 5, dtype=torch.int32))
    with pytest.raises(TypeError, match="color"):
        ops.model_intensity(None, torch.zeros(4, 5, dtype=torch.int64))


def test_provider_and_drivers():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam import ICPSLAM, PointFusion
    prov = ProjectiveICPOdometryProvider(color_weight=0.05)
    assert prov.color_weight == 0.05 and ProjectiveICPOdometryProvider().color_weight == 0.0
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)   # five keys
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="color_weight"):
            ProjectiveICPOdometryProvider(color_weight=bad)
    with pytest.raises(TypeError, match="color_weight"):
        ProjectiveICPOdometryProvider(color_weight="1")
    with pytest.raises(ValueError, match="differentiable"):
        ProjectiveICPOdometryProvider(color_weight=0.1, differentiable=True)
    assert ProjectiveICPOdometryProvider(color_weight=0.0, differentiable=True).differentiable
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, color_weight=0.2)
        assert s.color_weight == 0.2 and s.odomprov.color_weight == 0.2
        assert s.odomprov._kwargs() == dict(stride=2, numiters=20, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
        assert cls(odom="projicp").odomprov.color_weight == 0.0
        for odom in ("gt", "icp", "gradicp"):
            with pytest.raises(ValueError, match="color_weight"):
                cls(odom=odom, color_weight=0.1)
            assert cls(odom=odom, color_weight=0.0).color_weight == 0.0
        with pytest.raises(ValueError, match="color_weight"):
            cls(odom="projicp", color_weight=-1)
        with pytest.raises(ValueError, match="differentiable"):
            cls(odom="projicp", color_weight=0.1, odom_differentiable=True)
