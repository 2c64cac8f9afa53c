"""Tensor-level wrappers of the C-ABI (one sequence per call).  Each function validates
devices, allocates outputs with torch, and enqueues the HIP kernels on torch's current stream.
Nothing here computes with torch: arithmetic happens in libgradslam_hip.so or not at all."""
import collections
import math
import os

import torch

from . import _C
from ._C import Workspace, check, lib, ptr, require_device, stream

f32 = torch.float32

# True: the in-place SLAM drivers keep the surfel count of the map on the device between frames
# (the *_dc entry points) so that a frame never waits for a host read-back.  False: every count
# is read back as soon as it is produced (exact sizes on the host at all times).
DEVICE_COUNTS = os.environ.get("GRADSLAM_HIP_DEVICE_COUNTS", "1") != "0"


def _thresh(dist_thresh):
    """C-ABI encoding of dist_thresh: < 0 means None (no filter).  A negative USER threshold keeps no pair in the
    reference (squared distances are never below it, odometry/icputils.py:203-208); 0 has the same effect."""
    if dist_thresh is None:
        return -1.0
    return max(float(dist_thresh), 0.0)


def two_sigma_sq(sigma):
    if torch.is_tensor(sigma):
        sigma = float(sigma)
    return float(torch.tensor(2 * (float(sigma) ** 2), dtype=torch.float64).to(torch.float32))


def _c(t, dtype=f32):
    if t is None:
        return None
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


_IDENTITY4 = {}


def _identity4(dev):
    """read-only 4x4 identity of a device (the default initial transform of every ICP solve)"""
    t = _IDENTITY4.get(dev)
    if t is None:
        t = _IDENTITY4[dev] = torch.eye(4, dtype=f32, device=dev)
    return t


def _empty_rows(n, tail, dtype, dev):
    """torch.empty((n,) + tail) carved from an allocation whose row count is rounded up to a power of two: the
    per-frame temporaries sized by the (growing) surfel bound then change their allocation size only when the
    bound doubles, instead of asking the caching allocator for a slightly larger block every frame (each new
    size is a fresh hipMalloc while the host runs ahead of the device)."""
    cap = 1 << max(int(n) - 1, 0).bit_length() if n > 1024 else 1024
    return torch.empty((cap,) + tuple(tail), dtype=dtype, device=dev)[:n]


def _warn_detached(name, *tensors):
    """API functions without a backward kernel return detached tensors; say so instead of silently cutting the
    autograd graph (the reference's torch ops would have recorded it)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        import warnings
        warnings.warn("gradslam_amd.%s has no backward kernel: the result is detached from the autograd graph"
                      % name, RuntimeWarning, stacklevel=3)


def _count(t):
    """Reads a device int64 counter back (one host sync)."""
    return int(t.item())


# ----------------------------------------------------------------------------------- K1
def frame_maps(depth, K, sigma=0.6, want_normal=True, want_alpha=True, want_valid=True, out=None):
    """depth (H,W) f32, K (4,4) f32 -> vertex (H,W,3), normal (H,W,3), alpha (H,W), valid (H,W) bool.
    out: optional (vertex, normal, alpha) contiguous float32 buffers to write into (None entries are
    allocated / skipped according to the want_* flags)."""
    depth, K = _c(depth), _c(K)
    dev = require_device(depth, K)
    H, W = depth.shape
    ov, on, oa = out if out is not None else (None, None, None)
    vertex = ov if ov is not None else torch.empty((H, W, 3), dtype=f32, device=dev)
    normal = on if on is not None else (torch.empty((H, W, 3), dtype=f32, device=dev) if want_normal else None)
    alpha = oa if oa is not None else (torch.empty((H, W), dtype=f32, device=dev) if want_alpha else None)
    valid = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_valid else None
    require_device(vertex, normal, alpha)
    check(lib().gs_frame_maps_f32(ptr(depth), ptr(K), H, W, two_sigma_sq(sigma), ptr(vertex), ptr(normal),
                                  ptr(alpha), ptr(valid), stream(dev)), "gs_frame_maps_f32")
    return vertex, normal, alpha, (valid.view(torch.bool) if valid is not None else None)


def global_maps(vertex, normal, depth, pose, out=None):
    """out: optional (gvertex, gnormal) contiguous float32 buffers to write into."""
    vertex, normal, depth, pose = _c(vertex), _c(normal), _c(depth), _c(pose)
    dev = require_device(vertex, normal, depth, pose)
    H, W = depth.shape[:2]
    og, on = out if out is not None else (None, None)
    gv = og if og is not None else torch.empty_like(vertex)
    gn = on if on is not None else (torch.empty_like(normal) if normal is not None else None)
    require_device(gv, gn)
    check(lib().gs_global_maps_f32(ptr(vertex), ptr(normal), ptr(depth), ptr(pose), H, W, ptr(gv), ptr(gn),
                                   stream(dev)), "gs_global_maps_f32")
    return gv, gn


def _alpha_forward(points, sigma, eps):
    points = _c(points)
    dev = require_device(points)
    out = torch.empty(points.shape[:-1], dtype=f32, device=dev)
    check(lib().gs_alpha_f32(ptr(points), out.numel(), two_sigma_sq(sigma), float(eps), ptr(out), stream(dev)),
          "gs_alpha_f32")
    return out


class AlphaFunction(torch.autograd.Function):
    """get_alpha on an (n, 3) point array, differentiable w.r.t. the points and a tensor sigma
    (gs_alpha_backward_f32; the reference's own gradient check is tests/slam/test_fusionutils.py:56-75)."""

    @staticmethod
    def forward(ctx, points, sigma, eps):
        ctx.save_for_backward(points, sigma if torch.is_tensor(sigma) else None)
        ctx.sigma, ctx.eps = float(sigma), float(eps)
        return _alpha_forward(points, ctx.sigma, eps)

    @staticmethod
    def backward(ctx, a_bar):
        points, sigma_t = ctx.saved_tensors
        pts, a_bar = _c(points), _c(a_bar)
        dev = require_device(pts, a_bar)
        n = a_bar.numel()
        p_bar = torch.empty((n, 3), dtype=f32, device=dev)
        want_sigma = sigma_t is not None and ctx.needs_input_grad[1]
        terms = torch.empty(n, dtype=f32, device=dev) if want_sigma else None
        check(lib().gs_alpha_backward_f32(ptr(pts), n, two_sigma_sq(ctx.sigma), ctx.eps, ptr(a_bar), ptr(p_bar), ptr(terms),
                                          stream(dev)), "gs_alpha_backward_f32")
        s_bar = None
        if want_sigma:   # d alpha / d sigma = alpha |p|^2 / sigma^3, summed over the points in float64
            s_bar = (terms.double().sum() / (ctx.sigma ** 3)).to(sigma_t.dtype).reshape(sigma_t.shape).to(sigma_t.device)
        return p_bar.view(points.shape).to(points.dtype), s_bar, None


def alpha_of_points(points, sigma, eps=1e-7):
    """points (n, 3) -> alpha (n,); on the autograd tape when the points or a tensor sigma require grad."""
    if torch.is_grad_enabled() and (points.requires_grad or (torch.is_tensor(sigma) and sigma.requires_grad)):
        return AlphaFunction.apply(points, sigma, eps)
    return _alpha_forward(points, float(sigma), eps)


# ----------------------------------------------------------------------------------- K2
def downsample_frame(gvertex, gnormal, rgb, depth, ds, sync=True):
    """sync=False: no host read-back; returns the bound-sized buffers and the DEVICE count tensor
    (pts, nrm, col, count) for consumers that take device-side counts (icp(n_src_dev=...))."""
    gvertex, gnormal, rgb, depth = _c(gvertex), _c(gnormal), _c(rgb), _c(depth)
    dev = require_device(gvertex, gnormal, rgb, depth)
    H, W = depth.shape[:2]
    cap = ((H + ds - 1) // ds) * ((W + ds - 1) // ds)
    pts = torch.empty((cap, 3), dtype=f32, device=dev)
    nrm = torch.empty((cap, 3), dtype=f32, device=dev) if gnormal is not None else None
    col = torch.empty((cap, 3), dtype=f32, device=dev) if rgb is not None else None
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    check(lib().gs_downsample_frame_f32(ptr(gvertex), ptr(gnormal), ptr(rgb), ptr(depth), H, W, ds, ptr(pts),
                                        ptr(nrm), ptr(col), ptr(cnt), ptr(ws.scratch(0, H * W)), stream(dev)),
          "gs_downsample_frame_f32")
    if not sync:
        return pts, nrm, col, cnt
    c = _count(cnt)
    return pts[:c], (nrm[:c] if nrm is not None else None), (col[:c] if col is not None else None)


def lattice_source(vertex, depth, pose, ds):
    """ICP source of a frame without compaction: (ceil(H/ds)*ceil(W/ds), 3) global vertices of the lattice
    pixels, NaN where the pixel has no depth (ignored by icp's grid path)."""
    vertex, depth, pose = _c(vertex), _c(depth), _c(pose)
    dev = require_device(vertex, depth, pose)
    H, W = depth.shape[:2]
    out = torch.empty((-(-H // ds) * -(-W // ds), 3), dtype=f32, device=dev)
    check(lib().gs_lattice_source_f32(ptr(vertex), ptr(depth), ptr(pose), H, W, int(ds), ptr(out), stream(dev)),
          "gs_lattice_source_f32")
    return out


def project_map(points, pose, K, H, W, n_dev=None):
    """n_dev: device int64[1] holding the actual row count (points.shape[0] is then an upper bound)."""
    points, pose, K = _c(points), _c(pose), _c(K)
    dev = require_device(points, pose, K)
    n = points.shape[0]
    pix = _empty_rows(n, (), torch.int32, dev)
    if n_dev is not None:
        check(lib().gs_project_map_dc_f32(ptr(points), n, ptr(n_dev), ptr(pose), ptr(K), H, W, ptr(pix), stream(dev)),
              "gs_project_map_dc_f32")
        return pix
    check(lib().gs_project_map_f32(ptr(points), n, ptr(pose), ptr(K), H, W, ptr(pix), stream(dev)),
          "gs_project_map_f32")
    return pix


def active_table(pix, W, b=0):
    dev = require_device(pix)
    n = pix.shape[0]
    rows = torch.empty((n, 4), dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    check(lib().gs_active_table_i64(ptr(pix), n, W, b, ptr(rows), ptr(cnt), ptr(ws.scratch(n, 0)), stream(dev)),
          "gs_active_table_i64")
    return rows[: _count(cnt)]


def select_targets(pix, W, ds, points, normals, colors=None, cap=None, sync=True, n_dev=None):
    """sync=False: no host read-back; returns (pts, nrm, col, count) with bound-sized buffers."""
    points, normals, colors = _c(points), _c(normals), _c(colors)
    dev = require_device(pix, points, normals, colors)
    n = pix.shape[0]
    cap = n if cap is None else int(cap)
    op = _empty_rows(cap, (3,), f32, dev)
    on = _empty_rows(cap, (3,), f32, dev) if normals is not None else None
    oc = _empty_rows(cap, (3,), f32, dev) if colors is not None else None
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    if n_dev is not None:
        check(lib().gs_select_targets_dc_f32(ptr(pix), n, ptr(n_dev), W, ds, ptr(points), ptr(normals), ptr(colors),
                                             ptr(op), ptr(on), ptr(oc), cap, ptr(cnt), ptr(ws.scratch(n, 0)),
                                             stream(dev)), "gs_select_targets_dc_f32")
    else:
        check(lib().gs_select_targets_f32(ptr(pix), n, W, ds, ptr(points), ptr(normals), ptr(colors), ptr(op),
                                          ptr(on), ptr(oc), cap, ptr(cnt), ptr(ws.scratch(n, 0)), stream(dev)),
              "gs_select_targets_f32")
    if not sync:
        return op, on, oc, cnt
    c = _count(cnt)
    if c > cap:
        raise _C.HipExtensionError("gs_select_targets_f32: %d targets exceed capacity %d" % (c, cap))
    return op[:c], (on[:c] if on is not None else None), (oc[:c] if oc is not None else None)


def downsample_table(rows, ds, points, normals=None, colors=None):
    rows = _c(rows, torch.int64)
    points, normals, colors = _c(points), _c(normals), _c(colors)
    dev = require_device(rows, points, normals, colors)
    r = rows.shape[0]
    op = torch.empty((r, 3), dtype=f32, device=dev)
    on = torch.empty((r, 3), dtype=f32, device=dev) if normals is not None else None
    oc = torch.empty((r, 3), dtype=f32, device=dev) if colors is not None else None
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    check(lib().gs_downsample_table_f32(ptr(rows), r, ds, ptr(points), ptr(normals), ptr(colors), ptr(op), ptr(on),
                                        ptr(oc), ptr(cnt), ptr(ws.scratch(r, 0)), stream(dev)),
          "gs_downsample_table_f32")
    c = _count(cnt)
    return op[:c], (on[:c] if on is not None else None), (oc[:c] if oc is not None else None)


# ----------------------------------------------------------------------------------- K3 / K4
def knn1(src, tgt):
    src, tgt = _c(src), _c(tgt)
    dev = require_device(src, tgt)
    ns = src.shape[0]
    idx = torch.empty(ns, dtype=torch.int64, device=dev)
    d2 = torch.empty(ns, dtype=f32, device=dev)
    best = torch.empty(ns, dtype=torch.int64, device=dev)
    check(lib().gs_knn1_f32(ptr(src), ns, ptr(tgt), tgt.shape[0], ptr(idx), ptr(d2), ptr(best), stream(dev)),
          "gs_knn1_f32")
    return idx, d2


def knn1_grid(src, tgt, return_unresolved=False):
    """Same as knn1 through the uniform-grid engine used inside the ICP loop (bit-identical)."""
    import ctypes
    src, tgt = _c(src), _c(tgt)
    dev = require_device(src, tgt)
    ns, nt = src.shape[0], tgt.shape[0]
    idx = torch.empty(ns, dtype=torch.int64, device=dev)
    d2 = torch.empty(ns, dtype=f32, device=dev)
    scratch = Workspace.get(dev).bytes("knn_grid", lib().gs_knn1_grid_scratch_bytes(ns, nt))
    unres = ctypes.c_int64(0)
    check(lib().gs_knn1_grid_f32(ptr(src), ns, ptr(tgt), nt, ptr(idx), ptr(d2), ptr(scratch),
                                 ctypes.byref(unres) if return_unresolved else None, stream(dev)), "gs_knn1_grid_f32")
    return (idx, d2, unres.value) if return_unresolved else (idx, d2)


def gauss_newton_rows(src, tgt, tgt_normals, dist_thresh=None):
    src, tgt, tn = _c(src), _c(tgt), _c(tgt_normals)
    dev = require_device(src, tgt, tn)
    ns = src.shape[0]
    A = torch.empty((ns, 6), dtype=f32, device=dev)
    b = torch.empty(ns, dtype=f32, device=dev)
    idx = torch.empty(ns, dtype=torch.int64, device=dev)
    keep = torch.empty(ns, dtype=torch.uint8, device=dev)
    best = torch.empty(ns, dtype=torch.int64, device=dev)
    check(lib().gs_gauss_newton_rows_f32(ptr(src), ns, ptr(tgt), ptr(tn), tgt.shape[0],
                                         _thresh(dist_thresh), ptr(A), ptr(b),
                                         ptr(idx), ptr(keep), ptr(best), stream(dev)), "gs_gauss_newton_rows_f32")
    return A, b, idx, keep.view(torch.bool)


def solve_normal_eq(A, b, damp=1e-8, keep=None):
    A, b = _c(A), _c(b).reshape(-1)
    keep = None if keep is None else _c(keep.view(torch.uint8) if keep.dtype == torch.bool else keep, torch.uint8)
    dev = require_device(A, b, keep)
    x = torch.empty(A.shape[1], dtype=f32, device=dev)
    check(lib().gs_solve_normal_eq_f32(ptr(A), ptr(b), ptr(keep), A.shape[0], A.shape[1], float(damp), ptr(x),
                                       stream(dev)), "gs_solve_normal_eq_f32")
    return x


def _se3_exp_forward(xi):
    xi = _c(xi).reshape(6)
    dev = require_device(xi)
    T = torch.empty((4, 4), dtype=f32, device=dev)
    check(lib().gs_se3_exp_f32(ptr(xi), ptr(T), stream(dev)), "gs_se3_exp_f32")
    return T


class Se3ExpFunction(torch.autograd.Function):
    """se3_exp, differentiable w.r.t. xi (gs_se3_exp_backward_f32: the adjoint the ICP backward uses)."""

    @staticmethod
    def forward(ctx, xi):
        ctx.save_for_backward(xi)
        return _se3_exp_forward(xi)

    @staticmethod
    def backward(ctx, T_bar):
        (xi,) = ctx.saved_tensors
        x, T_bar = _c(xi).reshape(6), _c(T_bar)
        dev = require_device(x, T_bar)
        out = torch.empty(6, dtype=f32, device=dev)
        check(lib().gs_se3_exp_backward_f32(ptr(x), ptr(T_bar), ptr(out), stream(dev)), "gs_se3_exp_backward_f32")
        return out.view(xi.shape).to(xi.dtype)


def se3_exp(xi):
    if torch.is_grad_enabled() and xi.requires_grad:
        return Se3ExpFunction.apply(xi)
    return _se3_exp_forward(xi)


def lie_small(op, vec, n_in, n_out):
    """so3_hat (op 0) / se3_hat (1) / so3_exp (2) of a 3- / 6-vector (gs_lie_small_f32)."""
    _warn_detached(("so3_hat", "se3_hat", "so3_exp")[op], vec)
    v = _c(vec).reshape(n_in)
    dev = require_device(v)
    out = torch.empty((n_out, n_out), dtype=f32, device=dev)
    check(lib().gs_lie_small_f32(int(op), ptr(v), ptr(out), stream(dev)), "gs_lie_small_f32")
    return out


def project_points(cam, proj, pts_per_mat):
    """cam (n, 3|4), proj (m, 4, 4) with n = m * pts_per_mat -> (n, 2) (gs_project_points_f32)."""
    _warn_detached("project_points", cam, proj)
    cam, proj = _c(cam), _c(proj)
    dev = require_device(cam, proj)
    n = cam.shape[0]
    out = torch.empty((n, 2), dtype=f32, device=dev)
    check(lib().gs_project_points_f32(ptr(cam), int(cam.shape[1]), n, ptr(proj), int(pts_per_mat), ptr(out), stream(dev)),
          "gs_project_points_f32")
    return out


def unproject_points(pix, kinv, depths, pts_per_mat):
    """pix (n, 2|3), kinv (m, 3, 3), depths (n,) -> (n, 3) (gs_unproject_points_f32)."""
    _warn_detached("unproject_points", pix, kinv, depths)
    pix, kinv, depths = _c(pix), _c(kinv), _c(depths)
    dev = require_device(pix, kinv, depths)
    n = pix.shape[0]
    out = torch.empty((n, 3), dtype=f32, device=dev)
    check(lib().gs_unproject_points_f32(ptr(pix), int(pix.shape[1]), n, ptr(kinv), int(pts_per_mat), ptr(depths), ptr(out),
                                        stream(dev)), "gs_unproject_points_f32")
    return out


def ingest_depth(raw_u16, H, W, scale_div):
    """(H0, W0) uint16 depth as decoded from the PNG -> (H, W) float32 metres."""
    raw = raw_u16.contiguous()
    assert raw.dtype in (torch.uint16, torch.int16) and raw.ndim == 2
    dev = require_device(raw)
    out = torch.empty((H, W), dtype=f32, device=dev)
    check(lib().gs_ingest_depth_u16_f32(ptr(raw), raw.shape[0], raw.shape[1], ptr(out), H, W, float(scale_div),
                                        stream(dev)), "gs_ingest_depth_u16_f32")
    return out


def ingest_color(raw_u8, H, W, normalize=False):
    """(H0, W0, 3) uint8 colour -> (H, W, 3) float32 in [0, 255] (or [0, 1] when normalize)."""
    raw = raw_u8.contiguous()
    assert raw.dtype == torch.uint8 and raw.ndim == 3 and raw.shape[2] == 3
    dev = require_device(raw)
    out = torch.empty((H, W, 3), dtype=f32, device=dev)
    check(lib().gs_ingest_color_u8_f32(ptr(raw), raw.shape[0], raw.shape[1], ptr(out), H, W, 1 if normalize else 0,
                                       stream(dev)), "gs_ingest_color_u8_f32")
    return out


def host_device_pointer(t):
    """Device-side address of a PINNED host tensor (gs_host_device_pointer), or None when the allocation is not mapped
    into the device's address space."""
    import ctypes
    if t.is_cuda or not t.is_pinned():
        return None
    out = ctypes.c_void_p()
    rc = lib().gs_host_device_pointer(ctypes.c_void_p(t.data_ptr()), ctypes.byref(out))
    return out.value if rc == 0 and out.value else None


def ingest_frames_native(depth_raw, color_raw, depth_out, color_out, scale_div, normalize=False, on_stream=None):
    """n native-size raw frames -> float32 images in ONE launch (gs_ingest_frames_native_f32): depth_raw (..., H, W) uint16
    -> depth_out (same pixels) float32 metres, color_raw (..., H, W, 3) uint8 -> color_out float32; either pair may be
    None.  The raw tensors live on the device of the outputs -- or in PINNED host memory mapped into its address space
    (the kernel then reads them over PCIe: the streaming ingest).  `on_stream`: a torch stream to launch on (default:
    the current one)."""
    if (depth_raw is None) != (depth_out is None) or (color_raw is None) != (color_out is None) or \
            (depth_raw is None and color_raw is None):
        raise _C.HipExtensionError("ingest_frames_native: raw / out buffers must come in pairs (depth, colour or both)")
    if (depth_raw is not None and depth_raw.ndim < 2) or (color_raw is not None and (color_raw.ndim < 3 or color_raw.shape[-1] != 3)):
        raise _C.HipExtensionError("ingest_frames_native: raw / out buffers do not match")
    dev = require_device(depth_out if depth_raw is not None else color_out)
    H, W = (depth_raw.shape[-2:] if depth_raw is not None else color_raw.shape[-3:-1])
    n = (depth_raw.numel() if depth_raw is not None else color_raw.numel() // 3) // (H * W)
    ptrs = []
    for raw, out, dt, c in ((depth_raw, depth_out, (torch.uint16, torch.int16), 1), (color_raw, color_out, (torch.uint8,), 3)):
        if raw is None:
            ptrs += [None, None]
            continue
        if raw.dtype not in dt or out.dtype != f32 or not raw.is_contiguous() or not out.is_contiguous() or \
                out.numel() != raw.numel() or raw.numel() != n * H * W * c or out.device != dev:
            raise _C.HipExtensionError("ingest_frames_native: raw / out buffers do not match")
        if raw.is_cuda:
            if raw.device != dev:
                raise _C.HipExtensionError("ingest_frames_native: raw frames on another device")
            rp = raw.data_ptr()
        else:
            rp = host_device_pointer(raw)
            if rp is None:
                raise _C.HipExtensionError("ingest_frames_native: host frames must be pinned and device-mapped "
                                           "(tensor.pin_memory()); there is no CPU path")
        ptrs += [_C.C.c_void_p(rp), ptr(out)]
    st = stream(dev) if on_stream is None else _C.C.c_void_p(on_stream.cuda_stream)
    check(lib().gs_ingest_frames_native_f32(ptrs[0], ptrs[2], n, int(H), int(W), float(scale_div), 1 if normalize else 0,
                                            ptrs[1], ptrs[3], st), "gs_ingest_frames_native_f32")


def relative_pose(T01, T02):
    """(n, 4, 4) x (n, 4, 4) -> compose(inv(T01), T02) (relative_transformation of the reference)."""
    T01, T02 = _c(T01), _c(T02)
    dev = require_device(T01, T02)
    out = torch.empty_like(T02)
    check(lib().gs_relative_pose_f32(ptr(T01), ptr(T02), T02.numel() // 16, ptr(out), stream(dev)),
          "gs_relative_pose_f32")
    return out


def transform_points(pts, T):
    _warn_detached("transform_pointcloud", pts, T)
    pts, T = _c(pts), _c(T)
    dev = require_device(pts, T)
    out = torch.empty_like(pts)
    check(lib().gs_transform_points_f32(ptr(pts), pts.shape[0], ptr(T), ptr(out), stream(dev)),
          "gs_transform_points_f32")
    return out


def icp(src, tgt, tgt_normals, init=None, compose=None, mode=1, numiters=20, damp=1e-8, dist_thresh=None,
        lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, return_idx=True, return_trace=False, n_src_dev=None,
        n_tgt_dev=None, out=None):
    """Whole (grad)LM point-to-plane ICP on the device; returns T (4,4) [, idx (Ns,)] [, trace].
    n_src_dev / n_tgt_dev: device int64 tensors holding the actual point counts (the row counts of
    src / tgt are then upper bounds): nothing is read back to the host (gs_icp_dc_f32).
    out: optional contiguous (4, 4) float32 tensor that receives T."""
    src, tgt, tn = _c(src), _c(tgt), _c(tgt_normals)
    dev = require_device(src, tgt, tn)
    init = _identity4(dev) if init is None else _c(init)
    compose = _c(compose)
    require_device(init, compose)
    ns, nt = src.shape[0], tgt.shape[0]
    prm = _C.IcpParams(int(mode), int(numiters), float(damp), _thresh(dist_thresh),
                       float(lambda_max), float(B), float(B2), float(nu))
    T = torch.empty((4, 4), dtype=f32, device=dev) if out is None else out
    assert T.shape == (4, 4) and T.dtype == f32 and T.is_contiguous() and T.device == dev
    idx = torch.empty(ns, dtype=torch.int64, device=dev) if return_idx else None
    ws = Workspace.get(dev)
    dc = n_src_dev is not None or n_tgt_dev is not None
    scratch = ws.bytes("icp", lib().gs_icp_scratch_bytes(ns, nt))
    if dc:
        require_device(n_src_dev, n_tgt_dev)
        check(lib().gs_icp_dc_f32(ptr(src), ns, ptr(n_src_dev), ptr(tgt), ptr(tn), nt, ptr(n_tgt_dev), ptr(init),
                                  ptr(compose), prm, ptr(T), ptr(idx), ptr(scratch), stream(dev)), "gs_icp_dc_f32")
    else:
        check(lib().gs_icp_f32(ptr(src), ns, ptr(tgt), ptr(tn), nt, ptr(init), ptr(compose), prm, ptr(T), ptr(idx),
                               ptr(scratch), stream(dev)), "gs_icp_f32")
    out = [T]
    if return_idx:
        out.append(idx)
    if return_trace:
        tr = torch.empty((numiters, 12), dtype=f32, device=dev)
        check(lib().gs_icp_trace_f32(ptr(scratch), numiters, ptr(tr), stream(dev)), "gs_icp_trace_f32")
        out.append(tr)
    return out[0] if len(out) == 1 else tuple(out)


def icp_map(src, map_points, map_normals, pix, W, ds, n_map_dev=None, init=None, compose=None, mode=1, numiters=20,
            damp=1e-8, dist_thresh=None, lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, out=None):
    """(grad)LM ICP of `src` (NaN rows are skipped) against the map rows whose projection `pix` lies on the
    [::ds, ::ds] lattice, binned straight from the map (gs_icp_map_dc_f32): same T as select_targets + icp."""
    src, P, N = _c(src), _c(map_points), _c(map_normals)
    dev = require_device(src, P, N, pix)
    init = _identity4(dev) if init is None else _c(init)
    compose = _c(compose)
    require_device(init, compose, n_map_dev)
    ns, nm = src.shape[0], P.shape[0]
    prm = _C.IcpParams(int(mode), int(numiters), float(damp), _thresh(dist_thresh),
                       float(lambda_max), float(B), float(B2), float(nu))
    T = torch.empty((4, 4), dtype=f32, device=dev) if out is None else out
    assert T.shape == (4, 4) and T.dtype == f32 and T.is_contiguous() and T.device == dev
    scratch = Workspace.get(dev).bytes("icp", lib().gs_icp_scratch_bytes(ns, nm))
    check(lib().gs_icp_map_dc_f32(ptr(src), ns, None, ptr(P), ptr(N), ptr(pix), nm, ptr(n_map_dev), int(W), int(ds),
                                  ptr(init), ptr(compose), prm, ptr(T), ptr(scratch), stream(dev)), "gs_icp_map_dc_f32")
    return T


# ----------------------------------------------------------------------------------- K5
def similar_rows(rows, points, normals, gvertex, gnormal, dist_th, dot_th):
    rows = _c(rows, torch.int64)
    points, normals, gvertex, gnormal = _c(points), _c(normals), _c(gvertex), _c(gnormal)
    dev = require_device(rows, points, normals, gvertex, gnormal)
    W = gvertex.shape[1]
    mask = torch.empty(rows.shape[0], dtype=torch.uint8, device=dev)
    check(lib().gs_similar_rows_f32(ptr(rows), rows.shape[0], ptr(points), ptr(normals), ptr(gvertex), ptr(gnormal),
                                    W, float(dist_th), float(dot_th), ptr(mask), stream(dev)), "gs_similar_rows_f32")
    return mask.view(torch.bool)


def best_unique_rows(rows, points, ccounts, gvertex, b=0):
    rows = _c(rows, torch.int64)
    points, ccounts, gvertex = _c(points), _c(ccounts), _c(gvertex)
    dev = require_device(rows, points, ccounts, gvertex)
    H, W = gvertex.shape[:2]
    r = rows.shape[0]
    best = torch.empty(H * W, dtype=torch.int32, device=dev)
    out = torch.empty((H * W, 4), dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    check(lib().gs_best_unique_rows_f32(ptr(rows), r, ptr(points), ptr(ccounts), ptr(gvertex), H, W, b, ptr(best),
                                        ptr(out), ptr(cnt), ptr(ws.scratch(r, H * W)), stream(dev)),
          "gs_best_unique_rows_f32")
    return out[: _count(cnt)], best


def associate(pix, points, normals, ccounts, gvertex, gnormal, dist_th, dot_th, want_similar=False, n_dev=None):
    points, normals, ccounts, gvertex, gnormal = _c(points), _c(normals), _c(ccounts), _c(gvertex), _c(gnormal)
    dev = require_device(pix, points, normals, ccounts, gvertex, gnormal)
    H, W = gvertex.shape[:2]
    n = pix.shape[0]
    best = torch.empty(H * W, dtype=torch.int32, device=dev)
    sim = torch.empty(n, dtype=torch.uint8, device=dev) if want_similar else None
    ws = Workspace.get(dev)
    if n_dev is not None:
        check(lib().gs_associate_dc_f32(ptr(pix), n, ptr(n_dev), ptr(points), ptr(normals), ptr(ccounts),
                                        ptr(gvertex), ptr(gnormal), H, W, float(dist_th), float(dot_th), ptr(best),
                                        ptr(sim), ptr(ws.scratch(n, H * W)), stream(dev)), "gs_associate_dc_f32")
    else:
        check(lib().gs_associate_f32(ptr(pix), n, ptr(points), ptr(normals), ptr(ccounts), ptr(gvertex),
                                     ptr(gnormal), H, W, float(dist_th), float(dot_th), ptr(best), ptr(sim),
                                     ptr(ws.scratch(n, H * W)), stream(dev)), "gs_associate_f32")
    return (best, sim.view(torch.bool)) if want_similar else best


def best_table(best_pix, H, W, b=0):
    dev = require_device(best_pix)
    out = torch.empty((H * W, 4), dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    check(lib().gs_best_table_i64(ptr(best_pix), H, W, b, ptr(out), ptr(cnt), ptr(ws.scratch(0, H * W)),
                                  stream(dev)), "gs_best_table_i64")
    return out[: _count(cnt)]


def rows_to_best_pix(rows, H, W):
    rows = _c(rows, torch.int64)
    dev = require_device(rows)
    best = torch.empty(H * W, dtype=torch.int32, device=dev)
    check(lib().gs_rows_to_best_pix(ptr(rows), rows.shape[0], H, W, ptr(best), stream(dev)), "gs_rows_to_best_pix")
    return best


# ----------------------------------------------------------------------------------- K6
def fuse_append_(points, normals, colors, ccounts, n_map, best_pix, gvertex, gnormal, rgb, alpha, depth,
                 renorm_all=True, n_dev=None, sync=True):
    """In-place on capacity-backed buffers (rows >= n_map are free space).  Returns the new count
    (sync=False: as the device int64[1] tensor the kernels wrote, nothing is read back).
    n_dev: device-side count of the map (n_map is then its upper bound)."""
    gvertex, gnormal, rgb, alpha, depth = _c(gvertex), _c(gnormal), _c(rgb), _c(alpha), _c(depth)
    dev = require_device(points, normals, colors, ccounts, best_pix, gvertex, gnormal, rgb, alpha, depth)
    H, W = depth.shape[:2]
    cap = points.shape[0]
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    if n_dev is not None:
        check(lib().gs_fuse_append_dc_f32(ptr(points), ptr(normals), ptr(colors), ptr(ccounts), int(n_map),
                                          ptr(n_dev), cap, ptr(best_pix), ptr(gvertex), ptr(gnormal), ptr(rgb),
                                          ptr(alpha), ptr(depth), H, W, int(renorm_all), ptr(cnt),
                                          ptr(ws.scratch(n_map, H * W)), stream(dev)), "gs_fuse_append_dc_f32")
    else:
        check(lib().gs_fuse_append_f32(ptr(points), ptr(normals), ptr(colors), ptr(ccounts), int(n_map), cap,
                                       ptr(best_pix), ptr(gvertex), ptr(gnormal), ptr(rgb), ptr(alpha), ptr(depth),
                                       H, W, int(renorm_all), ptr(cnt), ptr(ws.scratch(n_map, H * W)),
                                       stream(dev)), "gs_fuse_append_f32")
    if not sync:
        return cnt
    c = _count(cnt)
    if c > cap:
        raise _C.HipExtensionError("gs_fuse_append_f32: surfel store overflow (%d > %d)" % (c, cap))
    return c


def update_map_fusion_(points, normals, colors, ccounts, n_map, vertex, normal, depth, rgb, alpha, pose, K, dist_th,
                       dot_th, renorm_all=True, n_dev=None, out=None):
    """One-call map update of a sequence (gs_update_map_fusion_dc_f32), in place on capacity-backed buffers.
    Returns (new count as a device int64[1] tensor, gvertex, gnormal, best_pix); nothing is read back."""
    vertex, normal, depth, rgb, alpha = _c(vertex), _c(normal), _c(depth), _c(rgb), _c(alpha)
    pose, K = _c(pose), _c(K)
    dev = require_device(points, normals, colors, ccounts, vertex, normal, depth, rgb, alpha, pose, K, n_dev)
    H, W = depth.shape[:2]
    cap = points.shape[0]
    gv, gn = out if out is not None else (torch.empty((H, W, 3), dtype=f32, device=dev),
                                          torch.empty((H, W, 3), dtype=f32, device=dev))
    best = torch.empty(H * W, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = Workspace.get(dev).bytes("map_update", lib().gs_update_map_scratch_bytes(int(n_map), H, W))
    check(lib().gs_update_map_fusion_dc_f32(ptr(points), ptr(normals), ptr(colors), ptr(ccounts), int(n_map), ptr(n_dev),
                                            cap, ptr(vertex), ptr(normal), ptr(depth), ptr(rgb), ptr(alpha), ptr(pose),
                                            ptr(K), H, W, float(dist_th), float(dot_th), 1 if renorm_all else 0, ptr(gv),
                                            ptr(gn), ptr(best), ptr(cnt), ptr(scratch), stream(dev)),
          "gs_update_map_fusion_dc_f32")
    return cnt, gv, gn, best


def append_valid_(points, normals, colors, ccounts, n_map, gvertex, gnormal, rgb, alpha, depth, n_dev=None,
                  sync=True):
    gvertex, gnormal, rgb, alpha, depth = _c(gvertex), _c(gnormal), _c(rgb), _c(alpha), _c(depth)
    dev = require_device(points, normals, colors, ccounts, gvertex, gnormal, rgb, alpha, depth)
    H, W = depth.shape[:2]
    cap = points.shape[0]
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    if n_dev is not None:
        check(lib().gs_append_valid_dc_f32(ptr(points), ptr(normals), ptr(colors), ptr(ccounts), int(n_map),
                                           ptr(n_dev), cap, ptr(gvertex), ptr(gnormal), ptr(rgb), ptr(alpha),
                                           ptr(depth), H, W, ptr(cnt), ptr(ws.scratch(n_map, H * W)), stream(dev)),
              "gs_append_valid_dc_f32")
    else:
        check(lib().gs_append_valid_f32(ptr(points), ptr(normals), ptr(colors), ptr(ccounts), int(n_map), cap,
                                        ptr(gvertex), ptr(gnormal), ptr(rgb), ptr(alpha), ptr(depth), H, W, ptr(cnt),
                                        ptr(ws.scratch(n_map, H * W)), stream(dev)), "gs_append_valid_f32")
    if not sync:
        return cnt
    c = _count(cnt)
    if c > cap:
        raise _C.HipExtensionError("gs_append_valid_f32: surfel store overflow (%d > %d)" % (c, cap))
    return c


# ----------------------------------------------------------------------------------- batched frame loop
def frame_maps_batch(depth, K, sigma=None, out=None):
    """K1 for every frame of a (B, L, H, W) depth stack in one launch (its (H, W) images must be contiguous; the
    sequence / frame strides are free, so a slice frames[:, s] of a longer stack is read in place): K (B, 4, 4) ->
    vertex (B, L, H, W, 3), normal (B, L, H, W, 3), alpha (B, L, H, W) or None (sigma None)."""
    K = _c(K)
    if depth.dtype != f32:
        depth = depth.to(f32)
    Bn, L, H, W = depth.shape
    if depth.stride(3) != 1 or depth.stride(2) != W or (L > 1 and depth.stride(1) < H * W) or \
            (Bn > 1 and depth.stride(0) < H * W):
        depth = depth.contiguous()
    dev = require_device(K)
    if depth.device != dev:
        raise _C.HipExtensionError("gradslam_amd kernels run on the GPU only; all tensors on one device")
    ov, on, oa = out if out is not None else (None, None, None)
    vertex = ov if ov is not None else torch.empty((Bn, L, H, W, 3), dtype=f32, device=dev)
    normal = on if on is not None else torch.empty((Bn, L, H, W, 3), dtype=f32, device=dev)
    alpha = oa if oa is not None else (torch.empty((Bn, L, H, W), dtype=f32, device=dev) if sigma is not None else None)
    require_device(vertex, normal, alpha)
    tss = two_sigma_sq(0.6 if sigma is None else sigma)
    sb, sl = (depth.stride(0) if Bn > 1 else L * H * W), (depth.stride(1) if L > 1 else H * W)
    step = max(32768 // L, 1) if Bn * L > 32768 and L <= 32768 else Bn   # gridDim.z limit: whole sequences per launch
    for b0 in range(0, Bn, step):
        m = min(step, Bn - b0)
        check(lib().gs_frame_maps_batch_f32(depth.data_ptr() + 4 * b0 * sb, sb, sl, ptr(K[b0:]), m * L, L, H, W, tss,
                                            ptr(vertex[b0:]), ptr(normal[b0:]),
                                            None if alpha is None else ptr(alpha[b0:]), stream(dev)),
              "gs_frame_maps_batch_f32")
    return vertex, normal, alpha


def _batch_view(t, inner_ndim):
    """(B, ...) float32 tensor whose per-sequence slices t[b] are contiguous -> (tensor kept alive, base pointer,
    batch stride in bytes).  A slice frames[:, s] of a (B, L, ...) stack qualifies as is (its batch stride is L
    frames): no copy; anything else is made contiguous first."""
    if t.dtype != f32:
        t = t.to(f32)
    inner = t.shape[t.ndim - inner_ndim:]
    want, acc = [], 1
    for d in reversed(inner):
        want.append(acc)
        acc *= int(d)
    if tuple(t.stride()[t.ndim - inner_ndim:]) != tuple(reversed(want)) or (t.shape[0] > 1 and t.stride(0) < acc):
        t = t.contiguous()
    return t, t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else acc) * 4


MapRows = collections.namedtuple("MapRows", ["points", "normals", "colors", "features", "n_bound", "n_dev"])
MapRows.__doc__ = """One sequence's map as every batched map pass takes it (`maps`: a list of these, or of tuples in this
order).  points (rows, 3), normals (rows, 3), colors (rows, 3), features (rows, F; a surfel map's confidence count: F = 1):
capacity-backed float32 buffers; an attribute the map lacks, or the pass does not read, may be None.  The first n_bound
rows are the map (None: every row).  n_dev: a device int64[1] tensor with the exact count -- n_bound is then its upper
bound on the host, a pass reads min(n_dev[0], n_bound) rows and nothing is read back -- or None when n_bound is exact.
The passes that read points and normals only (localize_batch, render_map_backward_batch, the projective ICP) also take the
short form (points, normals, n_bound, n_dev)."""
_MAP_ATTRS = MapRows._fields[:4]


def _map_rows(m, read=_MAP_ATTRS, four_ok=False):
    """One entry of `maps` (with four_ok also in the short form) -> the MapRows to take pointers from: the attributes named
    in `read` off the autograd tape and contiguous float32 (the tensor itself where it already is), the others None, and
    n_bound resolved against the rows of points.  What differs between the passes (shape refusals, negative bounds, the
    null pointers of empty maps) stays with them.  The result is also the keep-alive: a copy that had to be made lives
    here only, so an entry keeps the MapRows of ALL its sequences referenced until its launch is enqueued -- freed earlier,
    the caching allocator could hand the copy's block to a later sequence's output before the kernel has read it."""
    short = four_ok and len(m) == 4
    n_bound, n_dev = (m[2], m[3]) if short else (m[4], m[5])
    bufs = [None if t is None or k not in read else _c(t.detach() if t.requires_grad else t)
            for k, t in zip(_MAP_ATTRS, (m[0], m[1], None, None) if short else m[:4])]
    rows = int(bufs[0].shape[0]) if bufs[0] is not None and bufs[0].ndim else 0   # (no (rows, 3) points: the pass refuses)
    return MapRows(*bufs, rows if n_bound is None else min(int(n_bound), rows), n_dev)


def _map_view(m, *explicit):
    """the _C.MapView of a normalised MapRows (_map_rows): the only place one is built.  A caller that fills a descriptor
    by hand may pass the four buffers and spell out (capacity, n_bound, n_dev) after them."""
    cap, n_bound, n_dev = explicit or (m.points.shape[0], m.n_bound, m.n_dev)
    return _C.MapView(*[0 if t is None else t.data_ptr() for t in m[:4]], int(cap), int(n_bound),
                      0 if n_dev is None else n_dev.data_ptr())


def _seq_outs(who, out, spec, b, n_bound, dev):
    """The two per-sequence outputs of sequence b of a pass that marks rows; spec: their ((name, dtype), (name, dtype)).
    out None: new (n_bound,) tensors; else out[i][b], checked -- a list, or an entry of it, may be None (that output is
    then not produced), but not both of a sequence."""
    outs = []
    for i, (name, dtype) in enumerate(spec):
        if out is None:
            t = torch.empty((n_bound,), dtype=dtype, device=dev)
        else:
            t = None if out[i] is None else out[i][b]
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (n_bound,) or
                                  not t.is_contiguous()):
                raise ValueError("%s: out.%s[%d] must be a contiguous %s tensor of shape (%d,)"
                                 % (who, name, b, str(dtype).split(".")[-1], n_bound))
        outs.append(t)
    if outs[0] is None and outs[1] is None:
        raise ValueError("%s: out must ask for %s or %s (or both) of every map" % (who, spec[0][0], spec[1][0]))
    return outs


def _rows_bar(rows, width, n_bound, dev):
    """an uninitialised (rows, width) gradient buffer of a map attribute with the rows behind the bound zeroed: the
    backward kernels write the first n_bound rows"""
    g = torch.empty((rows, width), dtype=f32, device=dev)
    if n_bound < rows:
        g[n_bound:].zero_()
    return g


def localize_batch(vertex, depth, K, prev_poses, maps, ds, mode=1, numiters=20, damp=1e-8, dist_thresh=None,
                   lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, out=None):
    """ICPSLAM._localize for all sequences of a batch in one chain of launches (gs_localize_batch_f32).
    vertex (B, H, W, 3) LOCAL vertex maps of the live frames, depth (B, H, W), K / prev_poses (B, 4, 4);
    maps: per sequence a MapRows or its short form (points and normals are read).
    Returns the recovered poses (B, 4, 4) = T_icp @ prev_pose."""
    K, prev_poses = _c(K), _c(prev_poses)
    Bn, H, W = depth.shape
    vertex, v0, vs = _batch_view(vertex, 3)
    depth, d0, dstr = _batch_view(depth, 2)
    dev = require_device(K, prev_poses)
    if vertex.device != dev or depth.device != dev or not vertex.is_cuda:
        raise _C.HipExtensionError("gradslam_amd kernels run on the GPU only; all tensors on one device")
    T = torch.empty((Bn, 4, 4), dtype=f32, device=dev) if out is None else out
    assert T.shape == (Bn, 4, 4) and T.dtype == f32 and T.is_contiguous() and T.device == dev
    prm = _C.IcpParams(int(mode), int(numiters), float(damp), _thresh(dist_thresh), float(lambda_max), float(B),
                       float(B2), float(nu))
    ws = Workspace.get(dev)
    seqs = (_C.LocalizeSeq * Bn)()
    L = lib()
    k0, p0, t0 = K.data_ptr(), prev_poses.data_ptr(), T.data_ptr()
    for b in range(Bn):
        P, N = maps[b][0], maps[b][1]
        require_device(P, N, maps[b][-1])
        if P.dtype != f32 or N.dtype != f32 or N.shape[0] < P.shape[0]:
            raise _C.HipExtensionError("localize_batch needs float32 map points / normals on buffers of equal capacity "
                                       "(got %s / %s, %d / %d rows)" % (P.dtype, N.dtype, P.shape[0], N.shape[0]))
        m = _map_rows(maps[b], read=("points", "normals"), four_ok=True)   # (no copies: `maps` holds what is read)
        scratch = ws.bytes("localize%d" % b, L.gs_localize_scratch_bytes(H, W, int(ds), m.points.shape[0]))
        q = seqs[b]
        q.vertex, q.depth, q.K16, q.prev_pose16 = v0 + b * vs, d0 + b * dstr, k0 + b * 64, p0 + b * 64
        q.map = _map_view(m)
        q.out_pose16, q.scratch = t0 + b * 64, scratch.data_ptr()
    check(L.gs_localize_batch_f32(seqs, Bn, H, W, int(ds), prm, stream(dev)), "gs_localize_batch_f32")
    return T


def localize_list_stats(device, b, H, W, ds, capacity):
    """Diagnostics of the candidate lists of ordinary source points in the last localisation of sequence b on `device`
    (gs_localize_list_stats_i64): (failed[64], empty_list[64], without_list[64]) per launch of the solve (launch = 2 x
    iteration + half).  All zero when the solve kept no lists."""
    L = lib()
    scratch = Workspace.get(device).bytes("localize%d" % b, L.gs_localize_scratch_bytes(H, W, int(ds), int(capacity)))
    import ctypes
    out = (ctypes.c_int64 * 192)()
    check(L.gs_localize_list_stats_i64(scratch.data_ptr(), H, W, int(ds), int(capacity), out, stream(device)),
          "gs_localize_list_stats_i64")
    v = [int(x) for x in out]
    return v[:64], v[64:128], v[128:]


def localize_solve_stats(device, b, H, W, ds, capacity):
    """Diagnostics of the last localisation of sequence b on `device` (gs_localize_solve_stats_i64): {"weak": lists the
    list-building launch flagged as weak (GRADSLAM_HIP_ICP_WEAK_ROOM > 0)}."""
    L = lib()
    scratch = Workspace.get(device).bytes("localize%d" % b, L.gs_localize_scratch_bytes(H, W, int(ds), int(capacity)))
    import ctypes
    out = (ctypes.c_int64 * 8)()
    check(L.gs_localize_solve_stats_i64(scratch.data_ptr(), H, W, int(ds), int(capacity), out, stream(device)),
          "gs_localize_solve_stats_i64")
    return {"weak": int(out[3])}


def update_map_fusion_batch_(maps, vertex, normal, depth, rgb, alpha, poses, K, dist_th, dot_th, renorm_all=True,
                             out=None, want_best_pix=True):
    """update_map_fusion of all sequences of a batch, in place on their capacity-backed buffers
    (gs_update_map_fusion_batch_f32: 4 launches for the whole batch).  maps: per sequence a MapRows with all four
    attributes (features: the confidence count).  vertex / normal / rgb (B, H, W, 3), depth / alpha (B, H, W),
    poses / K (B, 4, 4).  Returns (counts int64 (B,) on the device, gvertex, gnormal, best_pix (B, H*W)).
    want_best_pix=False: the correspondence table is not written (the winners' scattered stores are saved) and the last
    element of the result is None; maps and counts are the same."""
    poses, K = _c(poses), _c(K)
    dev = require_device(poses, K)
    Bn, H, W = depth.shape
    views = [_batch_view(t, nd) for t, nd in ((vertex, 3), (normal, 3), (depth, 2), (rgb, 3), (alpha, 2))]
    if any(v[0].device != dev for v in views):
        raise _C.HipExtensionError("gradslam_amd kernels run on the GPU only; all tensors on one device")
    gv, gn = out if out is not None else (torch.empty((Bn, H, W, 3), dtype=f32, device=dev),
                                          torch.empty((Bn, H, W, 3), dtype=f32, device=dev))
    gviews = [_batch_view(t, 3) for t in (gv, gn)]
    assert gviews[0][0] is gv and gviews[1][0] is gn, "output global maps must have contiguous (H, W, 3) slices"
    best = torch.empty((Bn, H * W), dtype=torch.int32, device=dev) if want_best_pix else None
    cnt = torch.empty(Bn, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev)
    seqs = (_C.UpdateSeq * Bn)()
    L = lib()
    P1 = H * W * 4
    base = [None if t is None else t.data_ptr() for t in (poses, K, best, cnt)]
    for b in range(Bn):
        P, N, Cc, F, _, n_dev = maps[b]
        require_device(P, N, Cc, F, n_dev)   # (written in place: contiguous buffers, which _map_rows hands through)
        m = _map_rows(maps[b])
        scratch = ws.bytes("map_update%d" % b, L.gs_update_map_scratch_bytes(m.points.shape[0], H, W))
        u = seqs[b]
        u.map = _map_view(m)
        u.vertex, u.normal, u.depth, u.rgb, u.alpha = (v[1] + b * v[2] for v in views)
        u.pose16, u.K16 = base[0] + b * 64, base[1] + b * 64
        u.gvertex, u.gnormal = gviews[0][1] + b * gviews[0][2], gviews[1][1] + b * gviews[1][2]
        u.best_pix = None if best is None else base[2] + b * P1
        u.new_count_out, u.scratch = base[3] + b * 8, scratch.data_ptr()
    check(L.gs_update_map_fusion_batch_f32(seqs, Bn, H, W, float(dist_th), float(dot_th), 1 if renorm_all else 0,
                                           stream(dev)), "gs_update_map_fusion_batch_f32")
    return cnt, gv, gn, best


# ----------------------------------------------------------------------------------- surfel radii
def surfel_radius(depth, normal, K):
    """The radius of every depth sample as a surfel (gs_surfel_radius_f32; Keller et al.'s radius with ElasticFusion's
    cap on oblique surfaces): depth (..., H, W), normal (..., H, W, 3) the frames' LOCAL normal maps, K (..., 4, 4) one
    per image -> (radius (..., H, W) float32 in metres, valid (..., H, W) bool).  With fbar = (K[0,0] + K[1,1]) / 2:
    r0 = 0.70710678 z / fbar, radius = min(r0 / |n_z|, 2 r0); valid = z > 0 and a finite, non-zero normal; radius is 0
    where not valid.  A stack whose images are contiguous and evenly spaced (a slice frames[:, s] of a longer stack) is
    read in place."""
    who = "surfel_radius"
    if not (torch.is_tensor(depth) and torch.is_tensor(normal) and torch.is_tensor(K)):
        raise TypeError("%s: depth, normal and K must be tensors" % who)
    if depth.ndim < 2 or tuple(normal.shape) != tuple(depth.shape) + (3,) or \
            tuple(K.shape) != tuple(depth.shape[:-2]) + (4, 4):
        raise ValueError("%s: expected depth (..., H, W), normal (..., H, W, 3) and K (..., 4, 4); got %s, %s and %s"
                         % (who, tuple(depth.shape), tuple(normal.shape), tuple(K.shape)))
    _warn_detached(who, depth, normal, K)
    lead, (H, W) = tuple(depth.shape[:-2]), depth.shape[-2:]
    n = 1
    for d in lead:
        n *= int(d)

    def stack(t, inner):
        """(n, *inner) view of t with contiguous images, in place where its images are evenly spaced"""
        t = t.detach().to(f32)
        if len(lead) != 1:
            t = t.reshape((n,) + tuple(inner))   # (a view where the leading axes collapse to one stride, else a copy)
        want, acc = [], 1
        for d in reversed(inner):
            want.append(acc)
            acc *= int(d)
        if tuple(t.stride()[1:]) != tuple(reversed(want)) or (n > 1 and t.stride(0) < acc):
            t = t.contiguous()
        return t

    d2, n2, K2 = stack(depth, (H, W)), stack(normal, (H, W, 3)), _c(K.detach().reshape(n, 4, 4))
    dev = require_device(K2)
    if d2.device != dev or n2.device != dev:   # (strided stacks: contiguous per image, not as a whole)
        raise _C.HipExtensionError("gradslam_amd kernels run on the GPU only; all tensors on one device")
    radius = torch.empty(lead + (H, W), dtype=f32, device=dev)
    valid = torch.empty(lead + (H, W), dtype=torch.uint8, device=dev)
    if n:
        check(lib().gs_surfel_radius_f32(d2.data_ptr(), d2.stride(0) if n > 1 else H * W, n2.data_ptr(),
                                         n2.stride(0) if n > 1 else H * W * 3, ptr(K2), n, int(H), int(W), ptr(radius),
                                         ptr(valid), stream(dev)), "gs_surfel_radius_f32")
    return radius, valid.view(torch.bool)


# ----------------------------------------------------------------------------------- the model view
RenderedViews = collections.namedtuple("RenderedViews", ["depth", "color", "normal", "confidence", "index"])


RENDER_MAX_SPLAT = 8


def _render_radii(who, maps, radii, radius, max_radius):
    """The checks of the radii= / max_radius= pair of the model view, before anything else of the call (they need no
    GPU): radii None -> None; else the per-sequence (n_bound,) float32 tensors as given."""
    if isinstance(max_radius, bool) or not isinstance(max_radius, int):
        raise TypeError("%s: max_radius must be of type int; but was of type %s." % (who, type(max_radius)))
    if not 0 <= max_radius <= RENDER_MAX_SPLAT:
        raise ValueError("%s: max_radius (%d) must be 0 ... %d." % (who, max_radius, RENDER_MAX_SPLAT))
    if radii is None:
        return None
    if int(radius) != 0:
        raise ValueError("%s: radius (%d) must be 0 with radii: every row brings its own square (cap it with max_radius)"
                         % (who, int(radius)))
    if torch.is_tensor(radii) or len(radii) != len(maps):
        raise ValueError("%s: radii must be a list of one (N_b,) float32 tensor per sequence (%d)" % (who, len(maps)))
    for b, (r, m) in enumerate(zip(radii, maps)):
        rows = int(m[0].shape[0])
        bound = m[2] if len(m) == 4 else m[4]
        bound = rows if bound is None else min(int(bound), rows)
        if not torch.is_tensor(r) or r.dtype != f32:
            raise ValueError("%s: radii[%d] must be a float32 tensor; got %s"
                             % (who, b, r.dtype if torch.is_tensor(r) else type(r)))
        if r.ndim != 1 or int(r.shape[0]) != bound:
            raise ValueError("%s: radii[%d] must have shape (%d,), one radius per map row; got %s"
                             % (who, b, bound, tuple(r.shape)))
    return list(radii)


def _radii_pointers(radii, dev):
    """(host array of B device pointers, the tensors kept alive) of checked radii on `dev`"""
    held = [_c(r.detach()) for r in radii]
    if require_device(*held) not in (None, dev):
        raise _C.HipExtensionError("tensors live on different devices: %s vs %s" % (dev, held[0].device))
    import ctypes
    return (ctypes.c_void_p * len(held))(*[t.data_ptr() for t in held]), held


def render_map_batch(maps, poses, K, H, W, radius=0, min_confidence=0.0, cull_backfaces=False, out=None,
                     differentiable=False, guard=None, radii=None, max_radius=3):
    """The maps of B sequences seen from L poses each (gs_render_map_dc_f32: a z-buffered point render, one key launch
    and one resolve launch per 8 sequences x 4 views).  maps: per sequence a MapRows (features: the (rows, 1) confidence
    count); normals / colors / features may be None, the images that need them are then None.  poses (B, L, 4, 4)
    camera-to-world, K (B, 4, 4).  Returns RenderedViews(depth (B, L, H, W, 1), color (B, L, H, W, 3), normal (B, L, H,
    W, 3), confidence (B, L, H, W, 1), index (B, L, H, W) int64); pixels no row lands on hold 0 (index: -1).  out: a
    RenderedViews (or 5-tuple) of tensors to write into.
    radii: per sequence an (N_b,) float32 tensor of surfel radii in metres (ops.surfel_radius, a SurfelRadii layer): row n
    then competes for the (2 r + 1)^2 square of its own r = min(max_radius, floor(radii[n] * fbar / z)) (0 for a radius
    that is not positive and finite; fbar the mean focal length of K, z the row's depth in the view) through
    gs_render_map_radii_dc_f32; `radius` must be 0 and max_radius 0 ... 8.  The radii are constants of the gradient.
    differentiable=False: the result is detached (with a warning when an input requires grad).  differentiable=True:
    the four float images are on the autograd tape (RenderMapFunction per sequence: gradients reach the map rows and
    the poses, not K; index stays a plain tensor); `out` is then refused.  guard: see RenderMapFunction."""
    radii = _render_radii("render_map", maps, radii, radius, max_radius)
    if differentiable:
        if out is not None:
            raise ValueError("render_map: out= cannot be combined with differentiable=True (autograd owns the outputs)")
        if len(maps) != int(poses.shape[0]) or K.ndim != 3 or K.shape[0] != len(maps):
            raise ValueError("render_map: expected poses (B, L, 4, 4) and K (B, 4, 4) for B = %d maps; got %s and %s"
                             % (len(maps), tuple(poses.shape), tuple(K.shape)))
        poses = poses.to(f32)
        per = [RenderMapFunction.apply(m[0], m[1], m[2], m[3], poses[b], K[b].detach(), m[4], m[5], int(H), int(W),
                                       int(radius), float(min_confidence), bool(cull_backfaces), guard,
                                       None if radii is None else radii[b], max_radius)
               for b, m in enumerate(maps)]
        if any((per[0][i] is None) != (r[i] is None) for r in per for i in range(5)):
            raise ValueError("render_map: every map of a batch must carry the same attributes")
        return RenderedViews(*[None if per[0][i] is None else
                               (per[0][i].unsqueeze(0) if len(per) == 1 else torch.stack([r[i] for r in per]))
                               for i in range(5)])
    _warn_detached("render_map", poses, K, *[t for m in maps for t in m[:4]])
    poses, K = _c(poses.detach()), _c(K.detach())
    dev = require_device(poses, K)
    Bn, Lv = int(poses.shape[0]), int(poses.shape[1])
    H, W = int(H), int(W)
    if len(maps) != Bn or tuple(poses.shape[2:]) != (4, 4) or tuple(K.shape) != (Bn, 4, 4):
        raise ValueError("render_map: expected poses (B, L, 4, 4) and K (B, 4, 4) for B = %d maps; got %s and %s"
                         % (len(maps), tuple(poses.shape), tuple(K.shape)))
    if Lv == 0 or H <= 0 or W <= 0:
        raise ValueError("render_map: needs at least one view and a positive image size")
    held = [_map_rows(m) for m in maps]
    have = [all(h[i] is not None for h in held) for i in range(4)]
    if not have[0]:
        raise ValueError("render_map: a map without points")
    shapes = ((Bn, Lv, H, W, 1), (Bn, Lv, H, W, 3), (Bn, Lv, H, W, 3), (Bn, Lv, H, W, 1), (Bn, Lv, H, W))
    wanted = (True, have[2], have[1], have[3], True)
    imgs = []
    for i, (shape, want) in enumerate(zip(shapes, wanted)):
        t = None if out is None else out[i]
        if t is None and want:
            t = torch.empty(shape, dtype=torch.int64 if i == 4 else f32, device=dev)
        elif t is not None:
            if not want:
                raise ValueError("render_map: out.%s given but the maps lack the attribute it shows" % RenderedViews._fields[i])
            if tuple(t.shape) != shape or t.dtype != (torch.int64 if i == 4 else f32) or not t.is_contiguous():
                raise ValueError("render_map: out.%s must be a contiguous %s tensor of shape %s"
                                 % (RenderedViews._fields[i], "int64" if i == 4 else "float32", shape))
        imgs.append(t)
    require_device(*imgs)
    ws = Workspace.get(dev)
    L = lib()
    seqs = (_C.RenderSeq * Bn)()
    nbytes = L.gs_render_scratch_bytes(Lv, H, W)
    per_seq = [0 if t is None else t[0].numel() * t.element_size() for t in imgs]
    for b, m in enumerate(held):
        P = m.points
        require_device(*m[:4], m.n_dev, poses)
        if P.ndim != 2 or P.shape[1] != 3 or any(t is not None and t.shape[0] < P.shape[0] for t in m[1:4]):
            raise ValueError("render_map: points must be (rows, 3) and every attribute must hold as many rows")
        u = seqs[b]
        u.map = _map_view(m)
        u.poses16, u.K16 = poses.data_ptr() + b * Lv * 64, K.data_ptr() + b * 64
        u.depth, u.color, u.normal, u.confidence, u.index = (
            None if t is None else t.data_ptr() + b * sz for t, sz in zip(imgs, per_seq))
        u.scratch = ws.bytes("render%d" % b, nbytes).data_ptr()
    if radii is not None:
        rptr, rheld = _radii_pointers(radii, dev)
        check(L.gs_render_map_radii_dc_f32(seqs, rptr, Bn, Lv, H, W, max_radius, float(min_confidence),
                                           1 if cull_backfaces else 0, stream(dev)), "gs_render_map_radii_dc_f32")
        return RenderedViews(*imgs)
    check(L.gs_render_map_dc_f32(seqs, Bn, Lv, H, W, int(radius), float(min_confidence), 1 if cull_backfaces else 0,
                                 stream(dev)), "gs_render_map_dc_f32")
    return RenderedViews(*imgs)


def render_map(points, normals, colors, ccounts, poses, K, H, W, n_dev=None, radius=0, min_confidence=0.0,
               cull_backfaces=False, out=None, differentiable=False, radii=None, max_radius=3):
    """One map seen from L poses: render_map_batch for B = 1 without the batch dimension.  poses (L, 4, 4) or (4, 4),
    K (4, 4); n_dev: device int64[1] holding the actual row count (points.shape[0] is then an upper bound).  Returns
    RenderedViews(depth (L, H, W, 1), color (L, H, W, 3), normal (L, H, W, 3), confidence (L, H, W, 1), index (L, H, W)).
    radii: an (N,) float32 tensor, with max_radius; differentiable: see render_map_batch."""
    if poses.ndim == 2:
        poses = poses.unsqueeze(0)
    if out is not None:
        out = tuple(None if t is None else t.unsqueeze(0) for t in out)
    r = render_map_batch([(points, normals, colors, ccounts, None, n_dev)], poses.unsqueeze(0), K.reshape(1, 4, 4), H, W,
                         radius=radius, min_confidence=min_confidence, cull_backfaces=cull_backfaces, out=out,
                         differentiable=differentiable, radii=None if radii is None else [radii], max_radius=max_radius)
    return RenderedViews(*[None if t is None else t[0] for t in r])


# ----------------------------------------------------------------------------------- projective ICP
ProjectiveRows = collections.namedtuple("ProjectiveRows", ["code", "row", "a", "b", "sums", "count"])
PICP_TRACE = 8


def _picp_args(stride, numiters, damp, dist_thresh, angle_thresh):
    """the value checks of the projective ICP; returns (dist_th, dot_th) as the Python doubles the library casts"""
    for name, val in (("stride", stride), ("numiters", numiters)):
        if isinstance(val, bool) or not isinstance(val, int):
            raise TypeError("projective_icp: {} must be of type int; but was of type {}.".format(name, type(val)))
        if val < 1:
            raise ValueError("projective_icp: {} ({}) must be at least 1.".format(name, val))
    for name, val in (("damp", damp), ("dist_thresh", dist_thresh), ("angle_thresh", angle_thresh)):
        if isinstance(val, bool) or not isinstance(val, (float, int)):
            raise TypeError("projective_icp: {} must be of type float or int; but was of type {}.".format(name, type(val)))
        if math.isnan(val):
            raise ValueError("projective_icp: {} is NaN.".format(name))
    if not (damp > 0 and math.isfinite(damp)):
        raise ValueError("projective_icp: damp ({}) must be positive and finite.".format(damp))
    if not 0 <= angle_thresh <= 90:
        raise ValueError("projective_icp: angle_thresh ({}) must be within [0, 90] degrees.".format(angle_thresh))
    return float(dist_thresh), math.cos((angle_thresh * math.pi) / 180)


def _picp_number(who, name, val):
    """the value check of a Huber threshold (huber_delta: metres, color_huber_delta: intensity units), of a median rule's
    constant (huber_k, color_huber_k) and of the colour weight: a finite number >= 0, not a bool; 0 = off"""
    if isinstance(val, bool) or not isinstance(val, (float, int)):
        raise TypeError("{}: {} must be of type float or int; but was of type {}.".format(who, name, type(val)))
    if not (math.isfinite(val) and val >= 0):
        raise ValueError("{}: {} ({}) must be finite and not negative.".format(who, name, val))
    return float(val)


def _picp_huber(name, delta, who="projective_icp"):
    return _picp_number(who, name, delta)


def _picp_huber_k(huber_k, who="projective_icp"):
    """delta = huber_k * 1.4826 * median|b| per iteration; 0: huber_delta is the constant threshold it always was"""
    return _picp_number(who, "huber_k", huber_k)


def _picp_color_huber_k(color_huber_k, who, weight=None):
    """cdelta = color_huber_k * 1.4826 * median|r| per iteration; 0: color_huber_delta is the constant threshold it always
    was; weight: the colour weight of the call, without which there is no colour residual to estimate from"""
    color_huber_k = _picp_number(who, "color_huber_k", color_huber_k)
    if color_huber_k > 0 and weight is not None and not weight > 0:
        raise ValueError("{}: color_huber_k > 0 needs color_weight > 0: it estimates the Huber threshold of the colour "
                         "term".format(who))
    return color_huber_k


def _picp_color_weight(color_weight):
    """the colour weight (metres per intensity unit)"""
    return _picp_number("projective_icp_color", "color_weight", color_weight)


def _picp_flag(who, name, val):
    if not isinstance(val, bool):
        raise TypeError("{}: {} must be of type bool; but was of type {}.".format(who, name, type(val)))
    return val


def _picp_deterministic(who, name, val):
    """the type check of the ordered-backward switch: None (follow GRADSLAM_HIP_DETERMINISTIC_BACKWARD) or a bool"""
    if val is not None and not isinstance(val, bool):
        raise TypeError("{}: {} must be None or of type bool; but was of type {}.".format(who, name, type(val)))
    return val


PicpOptions = collections.namedtuple(
    "PicpOptions", ["stride", "numiters", "damp", "dist_th", "dot_th", "huber_delta", "huber_k", "color_weight",
                    "color_huber_delta", "color_huber_k", "deterministic"],
    defaults=(1, 1, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, None))
PicpOptions.__doc__ = """The validated options of a projective ICP call, as every layer below the public functions
carries them (_picp_solve, the autograd Functions, the backward, ProjectiveICPOdometryProvider): stride, numiters, damp
and the two gates as the library takes them (dist_th metres, dot_th = cos(angle_thresh)); the thresholds and median-rule
constants as floats, 0 = off; deterministic: None (the environment decides when the backward runs) or a bool."""


def _picp_options(who, base=None, flags=(), **given):
    """Validates into a PicpOptions on top of `base` (None: the defaults), IN THE ORDER THE KEYWORDS ARE WRITTEN: the order
    in which a bad call is refused belongs to each public function.  The keywords: geometry=(stride, numiters, damp,
    dist_thresh, angle_thresh), which goes through _picp_args; color_weight, huber_delta, huber_k, color_huber_delta,
    color_huber_k, deterministic; and the names in `flags`, bool switches of the caller's that are checked in their
    place and not kept.  Anything else is a mistake of the caller's.  color_huber_k > 0 needs color_weight > 0 where
    color_weight was validated earlier in the same call."""
    new = {}   # (one record is made, at the end: every _replace of a namedtuple is a microsecond of the call)
    for name, val in given.items():
        if name == "geometry":
            dist_th, dot_th = _picp_args(*val)
            new.update(stride=val[0], numiters=val[1], damp=float(val[2]), dist_th=dist_th, dot_th=dot_th)
        elif name in ("huber_delta", "huber_k", "color_huber_delta"):
            new[name] = _picp_number(who, name, val)
        elif name == "deterministic":
            new[name] = _picp_deterministic(who, name, val)
        elif name == "color_weight":
            new[name] = _picp_color_weight(val)
        elif name == "color_huber_k":
            new[name] = _picp_color_huber_k(val, who, new.get("color_weight"))
        elif name in flags:
            _picp_flag(who, name, val)
        else:
            raise TypeError("_picp_options: {!r} is neither an option nor one of the flags {}".format(name, flags))
    return PicpOptions(**new) if base is None else base._replace(**new)


def _picp_route(family, opt, weights=False, tape=False, ordered=False, tables=False):
    """Which export serves a call, and which sizer its scratch: (export, sizer), the library's names being
    gs_projective_icp_<export>_f32 and _PICP_SIZERS[sizer].  family: "batch", "rows", "color_batch", "color_rows" or
    "backward"; weights: pixel weights are given; tape: the forward fills a tape (batch only); ordered: the backward's
    ordered mode; tables: the optional per-slot output is asked for (rows: return_weights, backward:
    want_pixel_weights, which needs weights).  Per family the rungs in order, the first that holds serves the call:
    they are the features in the order they were added on top of each other -- the weighted entry serves every
    threshold, the scaled entries take huber_delta as the floor, the robust entries serve a tape as well."""
    k, ck = opt.huber_k > 0, opt.color_huber_k > 0
    delta, cdelta = opt.huber_delta > 0, opt.color_huber_delta > 0
    if (tape and family != "batch") or (ordered and family != "backward") or \
            (tables and not (family in ("rows", "color_rows") or (family == "backward" and weights))):
        raise ValueError("no projective ICP entry of family %r takes tape=%r, ordered=%r, tables=%r with weights=%r"
                         % (family, tape, ordered, tables, weights))
    if family == "batch":
        rungs = ((weights, "weighted_batch"), (k, "scaled_batch"), (delta, "robust_batch"), (tape, "tape_batch"),
                 (True, "batch"))
        sizer = "scaled" if k else "plain"
    elif family == "rows":
        rungs = ((weights, "weighted_rows"), (k, "scaled_rows"), (delta or tables, "robust_rows"), (True, "rows"))
        sizer = "scaled" if k else "plain"
    elif family == "color_batch":
        rungs = ((weights, "color_weighted_batch"), (ck, "color_joint_scaled_batch"), (k, "color_scaled_batch"),
                 (delta or cdelta, "color_robust_batch"), (True, "color_batch"))
        sizer = "joint_scaled" if ck or (weights and k) else "color_scaled" if k else "color"
    elif family == "color_rows":
        rungs = ((weights, "color_weighted_rows"), (k or ck, "color_joint_scaled_rows"),
                 (delta or cdelta or tables, "color_robust_rows"), (True, "color_rows"))
        sizer = "joint_scaled" if k or ck else "color"
    elif family == "backward":
        rungs = ((weights, "weighted_backward"), (ordered, "ordered_backward"), (k, "scaled_backward"),
                 (delta, "robust_backward"), (True, "backward"))
        sizer = "weighted_backward" if tables else "ordered_backward" if ordered else "backward"
    else:
        raise ValueError("no such family of projective ICP entries: %r" % (family,))
    for holds, export in rungs:
        if holds:
            return export, sizer


_PICP_SIZERS = {"plain": "gs_projective_icp_scratch_bytes", "scaled": "gs_projective_icp_scaled_scratch_bytes",
                "color": "gs_projective_icp_color_scratch_bytes",
                "color_scaled": "gs_projective_icp_color_scaled_scratch_bytes",
                "joint_scaled": "gs_projective_icp_color_joint_scaled_scratch_bytes",
                "backward": "gs_projective_icp_backward_scratch_bytes",
                "ordered_backward": "gs_projective_icp_ordered_backward_scratch_bytes",
                "weighted_backward": "gs_projective_icp_weighted_backward_scratch_bytes"}


def deterministic_backward_env():
    """GRADSLAM_HIP_DETERMINISTIC_BACKWARD as the library reads it for the grid-search ICP backward (gs_icp_bwd.hip),
    looked up on every call: on iff C atoi() of the value is nonzero (optional white space, an optional sign, then the
    leading decimal digits; no digits: 0)."""
    import os
    import re
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", os.environ.get("GRADSLAM_HIP_DETERMINISTIC_BACKWARD", ""))
    return m is not None and int(m.group(1)) != 0


PICP_NO_KEY = 0x7fffffff      # the key of a lattice slot that contributes nothing (the ordered backward's record)


def _picp_scale_table(Bn, numiters, dev):
    """the (B, numiters) table of thresholds of a scaled solve and its per-sequence device pointers"""
    scale = torch.empty((Bn, int(numiters)), dtype=f32, device=dev)
    return scale, (_C.C.c_void_p * Bn)(*[scale.data_ptr() + b * int(numiters) * 4 for b in range(Bn)])


def _picp_tensors(who, named):
    """every (name, value) of `named` is a tensor"""
    for name, t in named:
        if not torch.is_tensor(t):
            raise TypeError("{}: expected {} to be of type tensor; got {}".format(who, name, type(t)))


def _picp_nslots(H, W, stride):
    """slots of the [::stride, ::stride] lattice"""
    return ((H + stride - 1) // stride) * ((W + stride - 1) // stride)


def _picp_pixel_weights(who, pixel_weights, depth):
    """The checks of the per-pixel weights of a batched call against depth (B, H, W): a float32 tensor (B, H, W) on
    depth's device, or a list / tuple of B entries, each None (that sequence has no weights) or a float32 (H, W) tensor.
    Returns None (no weights at all) or the list of B entries, detached and contiguous.  The values are not looked at:
    a weight that is not a positive finite float32 masks its pixel on the device."""
    if pixel_weights is None:
        return None
    if not torch.is_tensor(depth) or depth.ndim != 3:
        return []   # (the checks of depth, which follow, refuse the call)
    Bn, H, W = (int(x) for x in depth.shape)
    if torch.is_tensor(pixel_weights):
        if tuple(pixel_weights.shape) != (Bn, H, W):
            raise ValueError("{}: expected pixel_weights of shape {} for depth {}; got {}".format(
                who, (Bn, H, W), tuple(depth.shape), tuple(pixel_weights.shape)))
        entries = [pixel_weights[b] for b in range(Bn)]
    elif isinstance(pixel_weights, (list, tuple)):
        if len(pixel_weights) != Bn:
            raise ValueError("{}: expected one pixel_weights entry per sequence ({}); got {}".format(
                who, Bn, len(pixel_weights)))
        entries = list(pixel_weights)
    else:
        raise TypeError("{}: expected pixel_weights to be of type tensor (or a list of tensors / None); got {}".format(
            who, type(pixel_weights)))
    out = []
    for t in entries:
        if t is None:
            out.append(None)
            continue
        if not torch.is_tensor(t):
            raise TypeError("{}: expected pixel_weights to be of type tensor; got {}".format(who, type(t)))
        if t.dtype != f32:
            raise TypeError("{}: pixel_weights must be float32; got {}".format(who, t.dtype))
        if tuple(t.shape) != (H, W):
            raise ValueError("{}: expected pixel_weights of shape {} per sequence; got {}".format(who, (H, W),
                                                                                                 tuple(t.shape)))
        if t.device != depth.device:
            raise ValueError("{}: pixel_weights must live on the inputs' device ({}); got {}".format(
                who, depth.device, t.device))
        out.append(t.detach().contiguous())
    return out


def _picp_weight_ptrs(entries):
    """the host array of B device pointers of _picp_pixel_weights' entries (NULL: that sequence has no weights)"""
    return (_C.C.c_void_p * len(entries))(*[None if t is None else t.data_ptr() for t in entries])


def _picp_seqs(who, vertex, normal, depth, K, index, model_poses, maps, init_poses):
    """Shape / dtype / device checks shared by the batched solve, the table-level call and the backward; fills the input
    fields of the descriptors (the scratch: _picp_scratch).  Returns (seqs, tensors kept alive, device, B, H, W)."""
    tensors = (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K), ("index", index),
               ("model_pose", model_poses), ("init_pose", init_poses))
    _picp_tensors(who, tensors)
    if depth.ndim != 3:
        raise ValueError("{}: expected depth (B, H, W); got {}".format(who, tuple(depth.shape)))
    Bn, H, W = (int(x) for x in depth.shape)
    want = {"vertex": (Bn, H, W, 3), "normal": (Bn, H, W, 3), "K": (Bn, 4, 4), "index": (Bn, H, W),
            "model_pose": (Bn, 4, 4), "init_pose": (Bn, 4, 4)}
    for name, t in tensors:
        if name in want and tuple(t.shape) != want[name]:
            raise ValueError("{}: expected {} of shape {} for depth {}; got {}".format(
                who, name, want[name], tuple(depth.shape), tuple(t.shape)))
    if Bn == 0 or H == 0 or W == 0 or len(maps) != Bn:
        raise ValueError("{}: needs at least one sequence, a positive image size and one map per sequence "
                         "(B = {}, {} maps)".format(who, Bn, len(maps)))
    if index.dtype != torch.int64:
        raise ValueError("{}: index must be the int64 index image of render_map; got {}".format(who, index.dtype))
    for m in maps:
        P, N = m[0], m[1]
        if P is None or N is None:
            raise ValueError("{}: a map without points or normals".format(who))
        if P.dtype != f32 or N.dtype != f32 or P.ndim != 2 or P.shape[1] != 3 or N.ndim != 2 or N.shape[1] != 3 or \
                N.shape[0] < P.shape[0] or not P.is_contiguous() or not N.is_contiguous():
            raise ValueError("{}: map points / normals must be contiguous float32 (rows, 3) tensors, normals with at "
                             "least as many rows as points (got {} {} / {} {})".format(
                                 who, P.dtype, tuple(P.shape), N.dtype, tuple(N.shape)))
    _warn_detached(who, vertex, normal, depth, K, model_poses, init_poses, *[t for m in maps for t in m[:2]])
    vertex, normal, depth, K, model_poses, init_poses = (_c(t.detach()) for t in (vertex, normal, depth, K, model_poses,
                                                                                  init_poses))
    index = index.contiguous()
    dev = require_device(vertex, normal, depth, K, index, model_poses, init_poses)
    held = [vertex, normal, depth, K, index, model_poses, init_poses]
    seqs = (_C.PicpSeq * Bn)()
    P3, P1 = H * W * 12, H * W * 4
    for b in range(Bn):
        m = _map_rows(maps[b], read=("points", "normals"), four_ok=True)   # (refused above unless float32, contiguous)
        require_device(m.points, m.normals, m.n_dev, vertex)
        if m.n_dev is not None and (m.n_dev.dtype != torch.int64 or m.n_dev.numel() < 1):
            raise ValueError("{}: the device count must be an int64 tensor".format(who))
        m = m._replace(n_bound=max(m.n_bound, 0))
        held.append(m)
        u = seqs[b]
        u.vertex, u.normal, u.depth = vertex.data_ptr() + b * P3, normal.data_ptr() + b * P3, depth.data_ptr() + b * P1
        u.K16, u.index, u.model_pose16 = K.data_ptr() + b * 64, index.data_ptr() + b * H * W * 8, \
            model_poses.data_ptr() + b * 64
        u.map = _map_view(m)
        u.init_pose16 = init_poses.data_ptr() + b * 64
    return seqs, held, dev, Bn, H, W


def _picp_scratch(seqs, dev, sizer, H, W, stride):
    """the forward's scratch of every sequence, from the workspace of the current stream; sizer: _picp_route's (the plain
    layout; "color": plus the colour-row counts; "scaled" / "color_scaled": plus the key table and the threshold of the
    median rule; "joint_scaled": plus the same again for the colour residual)"""
    ws = Workspace.get(dev)
    nbytes = getattr(lib(), _PICP_SIZERS[sizer])(H, W, int(stride))
    for b, u in enumerate(seqs):
        u.scratch = ws.bytes("picp%d" % b, nbytes).data_ptr()


def projective_icp_batch(vertex, normal, depth, K, index, model_poses, maps, init_poses, *, stride=1, numiters=10,
                         damp=1e-8, dist_thresh=0.1, angle_thresh=30.0, return_trace=False, out=None,
                         differentiable=False, guard=None, huber_delta=0.0, huber_k=0.0, return_scale=False,
                         deterministic=None, pixel_weights=None):
    """Frame-to-model tracking by projective data association for B sequences (gs_projective_icp_batch_f32: two launches
    per iteration for 8 sequences, nothing read back).  vertex / normal (B, H, W, 3): LOCAL maps of the live frames,
    depth (B, H, W), K (B, 4, 4); index (B, H, W) int64: the index image of render_map_batch at model_poses (B, 4, 4);
    maps: per sequence a MapRows or its short form (points and normals are read); init_poses (B, 4, 4).  Every lattice
    pixel [::stride, ::stride] with depth is carried by the current estimate into the model view and paired with the map
    row that won the pixel it lands on, if that row is within dist_thresh metres and angle_thresh degrees (normals);
    numiters point-to-plane Gauss-Newton steps with constant damping follow..  Returns the poses (B, 4, 4), detached; with
    return_trace also (B, numiters, 8) rows [inliers, sum of squared residuals, xi(6)]..  An iteration without inliers
    leaves the pose as it is.
    differentiable=True: the same pose bits, on the autograd tape (ProjectiveICPFunction: gradients reach vertex, the map
    points and normals and init_poses; the association, depth, K, model_poses and the live normals are constants);
    `out` is then refused.  guard: see ProjectiveICPFunction.
    huber_delta (metres, 0 = off): Huber weights (gs_projective_icp_robust_batch_f32): a used slot whose point-to-plane
    residual b exceeds it enters the normal equations with the weight huber_delta / |b|; the trace's second column is
    then the weighted sum of squares.  It works with differentiable=True (the weight is differentiated, which slots are
    clipped is a constant).
    huber_k (0 = off; 1.345 is the usual constant): the threshold is estimated from the residuals, per sequence and per
    iteration: delta = max(huber_k * 1.4826 * median|b|, huber_delta) with the lower median of |b| over the used slots at
    the pose the iteration linearises at (gs_projective_icp_scaled_batch_f32: two more launches per iteration, nothing
    read back, bit-exact); huber_delta is then a floor.  An iteration whose median is 0 has the plain solve's bits.  It
    works with differentiable=True (the thresholds are constants of the backward pass, like the clip flags).
    return_scale=True: the thresholds (B, numiters) float32 come last in the returned tuple (huber_k = 0: huber_delta in
    every entry).
    deterministic (None | bool; it means something with differentiable=True only): True makes the backward's map
    gradients bitwise reproducible (the ordered mode of projective_icp_backward_batch), False keeps the float64 atomics,
    None follows GRADSLAM_HIP_DETERMINISTIC_BACKWARD as read when the backward runs.
    pixel_weights (None = none: the entry points above run, the same bits): a float32 tensor (B, H, W) on the inputs'
    device, read at the pixel of each lattice slot (gs_projective_icp_weighted_batch_f32) -- a mask, a sensor model, a
    learned confidence.  A pixel whose weight is not a positive finite float32 (0, negative, NaN, +inf) is masked: it is
    not associated, not an inlier and in no median.  A used slot enters the normal equations with its pixel weight times
    its Huber weight (one float32 product); the trace's second column is the weighted sum of squares, the inlier count
    stays the number of used slots.  Weights of all ones give the bits of the call without weights; weight 0 on a set of
    pixels gives the bits of depth 0 there.  Nothing is validated on the host.  A list of B entries, each None (that
    sequence has no weights) or an (H, W) tensor, is taken as well.  With differentiable=True (the tensor form) the
    gradient reaches the weights too (WeightedProjectiveICPFunction; which pixels are masked is a constant), bitwise
    reproducible in both modes of the backward."""
    _picp_flag("projective_icp", "differentiable", differentiable)
    weights = _picp_pixel_weights("projective_icp", pixel_weights, depth)
    opt = _picp_options("projective_icp", deterministic=deterministic,
                        geometry=(stride, numiters, damp, dist_thresh, angle_thresh), huber_delta=huber_delta,
                        huber_k=huber_k, flags=("return_scale",), return_scale=return_scale)
    if not differentiable:
        return _picp_solve(opt, vertex, normal, depth, K, index, model_poses, maps, init_poses, out=out, weights=weights,
                           return_trace=return_trace, return_scale=return_scale)
    if out is not None:
        raise ValueError("projective_icp: out= cannot be combined with differentiable=True (autograd owns the "
                         "outputs)")
    return _picp_taped(opt, vertex, normal, depth, K, index, model_poses, maps, init_poses, pixel_weights, weights,
                       return_trace=return_trace, return_scale=return_scale, guard=guard)


PicpTapeConfig = collections.namedtuple("PicpTapeConfig", ["options", "counts", "guard"])
PicpTapeConfig.__doc__ = """the `cfg` of ProjectiveICPFunction / WeightedProjectiveICPFunction: the PicpOptions, per
sequence the map's (n_bound, n_dev), and the guard (a callable or None)"""


def _picp_taped(opt, vertex, normal, depth, K, index, model_poses, maps, init_poses, pixel_weights, weights, *,
                return_trace=False, return_scale=False, guard=None):
    """projective_icp_batch(differentiable=True) behind its value checks: the solve on the autograd tape; opt: the
    PicpOptions; weights: the entries of _picp_pixel_weights for pixel_weights"""
    cfg = PicpTapeConfig(opt, [(m[-2], m[-1]) for m in maps], guard)
    flat = [t for m in maps for t in m[:2]]
    if weights is not None and not torch.is_tensor(pixel_weights):
        raise ValueError("projective_icp: differentiable=True takes pixel_weights as one (B, H, W) tensor")
    if weights is not None:
        res = WeightedProjectiveICPFunction.apply(vertex, normal, depth, K, index, model_poses, init_poses,
                                                  pixel_weights, cfg, *flat)
    else:
        res = ProjectiveICPFunction.apply(vertex, normal, depth, K, index, model_poses, init_poses, cfg, *flat)
    scale = None
    if return_scale:
        scale = res[2] if opt.huber_k > 0 else torch.full_like(res[1][..., 0], opt.huber_delta)
    return _picp_pack(res[0], res[1], scale, return_trace, return_scale)


def _picp_pack(T, trace, scale, return_trace, return_scale):
    """what a solve returns: the poses, then the trace and the thresholds where asked for"""
    res = (T,) + ((trace,) if return_trace else ()) + ((scale,) if return_scale else ())
    return res if len(res) > 1 else T


def _picp_outputs(who, seqs, dev, out, return_trace, width, opt):
    """The outputs of a solve: `out` checked (or the poses allocated), the trace of `width` floats per iteration allocated
    when asked for, both wired into seqs (the PicpSeq of every sequence), and the PicpParams.  Returns (T, trace, prm)."""
    Bn = len(seqs)
    T = torch.empty((Bn, 4, 4), dtype=f32, device=dev) if out is None else out
    if tuple(T.shape) != (Bn, 4, 4) or T.dtype != f32 or not T.is_contiguous() or T.device != dev:
        raise ValueError("%s: out must be a contiguous float32 tensor of shape %s on %s" % (who, (Bn, 4, 4), dev))
    trace = torch.empty((Bn, opt.numiters, width), dtype=f32, device=dev) if return_trace else None
    for b, u in enumerate(seqs):
        u.out_pose16 = T.data_ptr() + b * 64
        u.trace = 0 if trace is None else trace.data_ptr() + b * opt.numiters * width * 4
    return T, trace, _C.PicpParams(*opt[:5])


def _picp_solve(opt, vertex, normal, depth, K, index, model_poses, maps, init_poses, *, color=None, model=None, out=None,
                tapes=None, weights=None, return_trace=False, return_scale=False, return_color_scale=False):
    """The batched solve of both families, geometric and (color, model given) joint, behind projective_icp_batch,
    projective_icp_color_batch and the autograd Functions' forward.  opt: the PicpOptions, which with `weights` (the
    entries of _picp_pixel_weights, or None) and `tapes` (None, or the uint8 (B, tape bytes) buffer a taped entry fills:
    the same kernels and pose bits) decides the entry (_picp_route).  Returns the poses, then the trace, the thresholds
    and the colour thresholds where asked for."""
    joint = color is not None
    who = "projective_icp_color" if joint else "projective_icp"
    export, sizer = _picp_route("color_batch" if joint else "batch", opt, weights=weights is not None,
                                tape=tapes is not None)
    seqs, held, dev, Bn, H, W = _picp_seqs(who, vertex, normal, depth, K, index, model_poses, maps, init_poses)
    _picp_scratch(seqs, dev, sizer, H, W, opt.stride)
    if joint:
        seqs = _picp_color_seqs(who, seqs, held, Bn, H, W, color, model)
    T, trace, prm = _picp_outputs(who, [c.base for c in seqs] if joint else list(seqs), dev, out, return_trace,
                                  PICP_COLOR_TRACE if joint else PICP_TRACE, opt)
    if weights is not None:
        require_device(*weights, held[0])
        held.append(weights)
        wptrs = _picp_weight_ptrs(weights)
    ptrs = None if tapes is None else \
        (_C.C.c_void_p * Bn)(*[tapes.data_ptr() + b * tapes.shape[1] for b in range(Bn)])
    # a table of thresholds is written only where it is asked for AND its median rule runs; else it is the constant
    scale, dptrs = _picp_scale_table(Bn, opt.numiters, dev) if return_scale and opt.huber_k > 0 else (None, None)
    cscale, cptrs = _picp_scale_table(Bn, opt.numiters, dev) if return_color_scale and opt.color_huber_k > 0 \
        else (None, None)
    L, st = lib(), stream(dev)
    delta, k, cw, cdelta, ck = opt.huber_delta, opt.huber_k, opt.color_weight, opt.color_huber_delta, opt.color_huber_k
    # (the scaled entries take (k, floor), the weighted ones (delta, k))
    if export == "weighted_batch":
        status = L.gs_projective_icp_weighted_batch_f32(seqs, wptrs, ptrs, dptrs, Bn, H, W, prm, delta, k, st)
    elif export == "scaled_batch":
        status = L.gs_projective_icp_scaled_batch_f32(seqs, ptrs, dptrs, Bn, H, W, prm, k, delta, st)
    elif export == "robust_batch":
        status = L.gs_projective_icp_robust_batch_f32(seqs, ptrs, Bn, H, W, prm, delta, st)
    elif export == "tape_batch":
        status = L.gs_projective_icp_tape_batch_f32(seqs, ptrs, Bn, H, W, prm, st)
    elif export == "batch":
        status = L.gs_projective_icp_batch_f32(seqs, Bn, H, W, prm, st)
    elif export == "color_weighted_batch":
        status = L.gs_projective_icp_color_weighted_batch_f32(seqs, wptrs, dptrs, cptrs, Bn, H, W, prm, cw, delta, k,
                                                              cdelta, ck, st)
    elif export == "color_joint_scaled_batch":
        status = L.gs_projective_icp_color_joint_scaled_batch_f32(seqs, dptrs, cptrs, Bn, H, W, prm, cw, k, delta, ck,
                                                                  cdelta, st)
    elif export == "color_scaled_batch":
        status = L.gs_projective_icp_color_scaled_batch_f32(seqs, dptrs, Bn, H, W, prm, cw, k, delta, cdelta, st)
    elif export == "color_robust_batch":
        status = L.gs_projective_icp_color_robust_batch_f32(seqs, Bn, H, W, prm, cw, delta, cdelta, st)
    else:
        status = L.gs_projective_icp_color_batch_f32(seqs, Bn, H, W, prm, cw, st)
    check(status, "gs_projective_icp_%s_f32" % export)
    if return_scale and scale is None:
        scale = torch.full((Bn, opt.numiters), delta, dtype=f32, device=dev)
    if return_color_scale and cscale is None:
        cscale = torch.full((Bn, opt.numiters), cdelta, dtype=f32, device=dev)
    res = _picp_pack(T, trace, scale, return_trace, return_scale)
    if return_color_scale:
        res = (res if isinstance(res, tuple) else (res,)) + (cscale,)
    return res


def projective_icp_tape_bytes(numiters):
    """bytes of one sequence's forward tape (328 per iteration: the pose, the 28 sums, the step, the inlier count)"""
    return int(lib().gs_projective_icp_tape_bytes(int(numiters)))


def projective_icp_backward_batch(vertex, normal, depth, K, index, model_poses, maps, tapes, pose_bar, *, stride=1,
                                  numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0, want_vertex=True,
                                  want_init=True, want_maps=None, huber_delta=0.0, huber_k=0.0, deterministic=None,
                                  return_contributions=False, pixel_weights=None, want_pixel_weights=False):
    """Reverse mode of projective_icp_batch (gs_projective_icp_backward_batch_f32), arguments as the forward's; tapes:
    the (B, projective_icp_tape_bytes(numiters)) uint8 buffer the taped forward filled; pose_bar (B, 4, 4): the adjoint of
    the poses.  want_maps: per sequence (points, normals) flags, default all True.  Returns (vertex_bar (B, H, W, 3) or
    None, per sequence (points_bar, normals_bar) of the buffers' shapes (None where not wanted), init_pose_bar (B, 4, 4)
    or None).  vertex_bar and init_pose_bar are bitwise reproducible, the map gradients up to the order of float64
    additions.  An output that is not wanted costs nothing: without map outputs nothing of map size is allocated.
    huber_delta: the threshold the taped forward ran with (gs_projective_icp_robust_backward_batch_f32 when > 0).
    huber_k > 0: the taped forward ran with the median rule (gs_projective_icp_scaled_backward_batch_f32): every
    iteration's threshold is read from the tape and is a constant of the pass; huber_delta is then not read.
    deterministic=True: the ordered mode (gs_projective_icp_ordered_backward_batch_f32, for all three tapes): the map
    gradients are bitwise reproducible too -- every slot's contribution is recorded next to its row, the records are
    stable-sorted by row and added per row in ascending slot order, iteration by iteration; vertex_bar and init_pose_bar
    keep their bits.  False: the atomic mode.  None: GRADSLAM_HIP_DETERMINISTIC_BACKWARD decides, read at this call
    (deterministic_backward_env).  return_contributions=True (ordered mode only): a fourth result, per sequence (keys
    (numiters, nslots) int32, contrib (numiters, nslots, 6) float64): the record of every iteration as the kernel wrote it,
    keys = the slot's row or PICP_NO_KEY, contrib = its contributions to points_bar[row] and normals_bar[row] (defined
    where the key is a row).
    pixel_weights: the weights the taped forward ran with (as in projective_icp_batch; None: it ran without).  The
    result then has one more entry, LAST: pixel_weights_bar (B, H, W) float32 with want_pixel_weights=True, else None
    (nothing is allocated or computed for it).  It is accumulated per slot in float64 by the slot's own thread and rounded
    once: bitwise reproducible, and the same bits in the atomic and the ordered mode; +0.0 off the lattice, at masked
    pixels and at pixels never used (gs_projective_icp_weighted_backward_batch_f32)."""
    who = "projective_icp_backward"
    flags = ("want_pixel_weights", "return_contributions")
    opt = _picp_options(who, geometry=(stride, numiters, damp, dist_thresh, angle_thresh), flags=flags,
                        want_pixel_weights=want_pixel_weights)
    weights = _picp_pixel_weights(who, pixel_weights, depth)
    if want_pixel_weights and weights is None:
        raise ValueError("projective_icp_backward: want_pixel_weights=True needs the pixel_weights of the forward")
    opt = _picp_options(who, opt, huber_delta=huber_delta, huber_k=huber_k, deterministic=deterministic, flags=flags,
                        return_contributions=return_contributions)
    return _picp_backward(opt, vertex, normal, depth, K, index, model_poses, maps, tapes, pose_bar,
                          want_vertex=want_vertex, want_init=want_init, want_maps=want_maps, weights=weights,
                          want_pixel_weights=want_pixel_weights, return_contributions=return_contributions)


def _picp_backward(opt, vertex, normal, depth, K, index, model_poses, maps, tapes, pose_bar, *, want_vertex, want_init,
                   want_maps, weights=None, want_pixel_weights=False, return_contributions=False):
    """projective_icp_backward_batch behind its value checks; opt: the PicpOptions of the taped forward; weights: the
    entries of _picp_pixel_weights (None: the forward ran without)"""
    ordered = deterministic_backward_env() if opt.deterministic is None else opt.deterministic
    if return_contributions and not ordered:
        raise ValueError("projective_icp_backward: return_contributions=True needs the ordered mode (deterministic=True "
                         "or GRADSLAM_HIP_DETERMINISTIC_BACKWARD=1)")
    weighted = weights is not None
    export, sizer = _picp_route("backward", opt, weights=weighted, ordered=ordered, tables=want_pixel_weights)
    with torch.no_grad():
        seqs, held, dev, Bn, H, W = _picp_seqs("projective_icp_backward", vertex, normal, depth, K, index, model_poses,
                                               maps, pose_bar)
    numiters, stride = opt.numiters, opt.stride
    if not torch.is_tensor(tapes) or tapes.dtype != torch.uint8 or tapes.ndim != 2 or not tapes.is_contiguous() or \
            tuple(tapes.shape) != (Bn, projective_icp_tape_bytes(numiters)) or tapes.device != dev:
        raise ValueError("projective_icp_backward: tapes must be the contiguous uint8 (B, %d) buffer of the taped forward"
                         % projective_icp_tape_bytes(numiters))
    want_maps = [(True, True)] * Bn if want_maps is None else [tuple(bool(x) for x in w) for w in want_maps]
    if len(want_maps) != Bn:
        raise ValueError("projective_icp_backward: want_maps needs one (points, normals) pair per sequence")
    pose_bar = held[6]   # (contiguous float32, as _picp_seqs made it)
    vertex_bar = torch.empty((Bn, H, W, 3), dtype=f32, device=dev) if want_vertex else None
    init_bar = torch.empty((Bn, 4, 4), dtype=f32, device=dev) if want_init else None
    ws = Workspace.get(dev)
    L = lib()
    # (the weighted entry takes the ordered descriptors in both modes)
    oseqs = (_C.PicpOrderedBackwardSeq * Bn)() if export in ("weighted_backward", "ordered_backward") else None
    bseqs = (_C.PicpBackwardSeq * Bn)() if oseqs is None else None
    # (the weighted sizer: the float64 accumulator of pixel_weights_bar, 8 bytes per slot more, in either mode)
    size, mode = getattr(L, _PICP_SIZERS[sizer]), ((1 if ordered else 0,) if sizer == "weighted_backward" else ())
    if weighted:
        require_device(*weights, held[0])
    weights_bar = torch.empty((Bn, H, W), dtype=f32, device=dev) if want_pixel_weights else None
    nslots = _picp_nslots(H, W, stride)
    rows_out, record = [], []
    for b in range(Bn):
        u, f = oseqs[b].base if oseqs is not None else bseqs[b], seqs[b]
        u.vertex, u.normal, u.depth, u.K16, u.index, u.model_pose16 = f.vertex, f.normal, f.depth, f.K16, f.index, \
            f.model_pose16
        u.map = f.map
        P, N = maps[b][0], maps[b][1]
        n_bound = int(f.map.n_bound)
        outs = [_rows_bar(int(t.shape[0]), 3, n_bound, dev) if w else None for t, w in zip((P, N), want_maps[b])]
        rows_out.append(tuple(outs))
        u.tape = tapes.data_ptr() + b * tapes.shape[1]
        u.pose_bar16 = pose_bar.data_ptr() + b * 64
        u.vertex_bar = None if vertex_bar is None else vertex_bar.data_ptr() + b * H * W * 12
        u.points_bar, u.normals_bar = (None if g is None else g.data_ptr() for g in outs)
        u.init_pose_bar16 = None if init_bar is None else init_bar.data_ptr() + b * 64
        buf = ws.bytes("picp_bwd%d" % b, size(H, W, stride, n_bound if any(want_maps[b]) else 0, *mode))
        u.scratch, u.scratch_bytes = buf.data_ptr(), int(buf.numel())
        if return_contributions:   # (what the kernel does not write reads "none" / zero)
            keys = torch.full((numiters, nslots), PICP_NO_KEY, dtype=torch.int32, device=dev)
            contrib = torch.zeros((numiters, nslots, 6), dtype=torch.float64, device=dev)
            oseqs[b].key_out, oseqs[b].contrib_out = keys.data_ptr(), contrib.data_ptr()
            record.append((keys, contrib))
    prm = _C.PicpParams(stride, numiters, opt.damp, opt.dist_th, opt.dot_th)
    sort_buf = None
    if ordered:
        sort_bytes = L.gs_projective_icp_ordered_backward_sort_scratch_bytes(Bn, H, W, stride)
        if sort_bytes <= 0:
            raise ValueError("projective_icp_backward: the lattices of a launch group (%d x %d slots) are too many for "
                             "one sort of the ordered mode" % (min(Bn, 8), nslots))
        sort_buf = ws.bytes("picp_bwd_sort", sort_bytes) if any(any(w) for w in want_maps) else None
    sort_ptr, sort_len = (None, 0) if sort_buf is None else (sort_buf.data_ptr(), int(sort_buf.numel()))
    # (a scaled tape holds every iteration's threshold: huber_delta is then not read)
    delta, scaled = (0.0, 1) if opt.huber_k > 0 else (opt.huber_delta, 0)
    st = stream(dev)
    if export == "weighted_backward":
        bar_ptrs = None if weights_bar is None else \
            (_C.C.c_void_p * Bn)(*[weights_bar.data_ptr() + b * H * W * 4 for b in range(Bn)])
        status = L.gs_projective_icp_weighted_backward_batch_f32(oseqs, _picp_weight_ptrs(weights), bar_ptrs, Bn, H, W,
                                                                 prm, delta, scaled, 1 if ordered else 0, sort_ptr,
                                                                 sort_len, st)
    elif export == "ordered_backward":
        status = L.gs_projective_icp_ordered_backward_batch_f32(oseqs, Bn, H, W, prm, delta, scaled, sort_ptr, sort_len,
                                                                st)
    elif export == "scaled_backward":
        status = L.gs_projective_icp_scaled_backward_batch_f32(bseqs, Bn, H, W, prm, st)
    elif export == "robust_backward":
        status = L.gs_projective_icp_robust_backward_batch_f32(bseqs, Bn, H, W, prm, opt.huber_delta, st)
    else:
        status = L.gs_projective_icp_backward_batch_f32(bseqs, Bn, H, W, prm, st)
    check(status, "gs_projective_icp_%s_batch_f32" % export)
    res = (vertex_bar, rows_out, init_bar) + ((record,) if return_contributions else ())
    return res + (weights_bar,) if weighted else res


def _picp_taped_forward(ctx, tensors, cfg, flat):
    """the forward of both autograd Functions; tensors: the inputs in front of cfg (vertex, normal, depth, K, index,
    model_poses, init_poses, and the pixel weights of the weighted Function)"""
    depth, opt = tensors[2], cfg.options
    maps = [(flat[2 * b], flat[2 * b + 1]) + tuple(cfg.counts[b]) for b in range(len(flat) // 2)]
    tapes = torch.empty((int(depth.shape[0]), projective_icp_tape_bytes(opt.numiters)), dtype=torch.uint8,
                        device=depth.device)
    weights = _picp_pixel_weights("projective_icp", tensors[7], depth) if len(tensors) > 7 else None
    res = _picp_solve(opt, *tensors[:6], maps, tensors[6], tapes=tapes, weights=weights, return_trace=True,
                      return_scale=opt.huber_k > 0)
    ctx.save_for_backward(*tensors[:6], tapes, *tensors[7:], *flat, *[c[1] for c in cfg.counts])
    # (opt.deterministic None: the backward reads GRADSLAM_HIP_DETERMINISTIC_BACKWARD when it runs, not now)
    ctx.opt, ctx.bounds, ctx.guard = opt, [c[0] for c in cfg.counts], cfg.guard
    ctx.mark_non_differentiable(*res[1:])
    return res


def _picp_taped_backward(ctx, T_bar, weighted):
    """the backward of both autograd Functions; weighted: input 7 is the pixel weights (cfg and the maps follow it)"""
    if ctx.guard is not None:
        ctx.guard()
    n_in = 9 if weighted else 8   # (the inputs in front of the maps' tensors, cfg among them)
    saved, Bn, need = ctx.saved_tensors, len(ctx.bounds), ctx.needs_input_grad
    flat, n_devs = saved[n_in - 1:n_in - 1 + 2 * Bn], saved[n_in - 1 + 2 * Bn:]
    want_maps = [(bool(need[n_in + 2 * b]), bool(need[n_in + 1 + 2 * b])) for b in range(Bn)]
    if T_bar is None or not (need[0] or need[6] or (weighted and need[7]) or any(any(w) for w in want_maps)):
        return (None,) * (n_in + 2 * Bn)
    maps = [(flat[2 * b], flat[2 * b + 1], ctx.bounds[b], n_devs[b]) for b in range(Bn)]
    weights = _picp_pixel_weights("projective_icp_backward", saved[7], saved[2]) if weighted else None
    res = _picp_backward(ctx.opt, *saved[:6], maps, saved[6], T_bar, want_vertex=bool(need[0]), want_init=bool(need[6]),
                         want_maps=want_maps, weights=weights, want_pixel_weights=weighted and bool(need[7]))
    return (res[0], None, None, None, None, None, res[2]) + ((res[3], None) if weighted else (None,)) + \
        tuple(g for r in res[1] for g in r)


class ProjectiveICPFunction(torch.autograd.Function):
    """projective_icp_batch on the autograd tape: forward = gs_projective_icp_tape_batch_f32 (the plain solve's kernels
    and pose bits, plus the tape), backward = one call of gs_projective_icp_backward_batch_f32.  Inputs: vertex, normal,
    depth, K, index, model_poses, init_poses, cfg (the keyword arguments, `counts` = per sequence (n_bound, n_dev),
    `guard` and optionally `huber_delta`: both passes then run the robust entries, or `huber_k`: the scaled entries, and
    the thresholds (B, numiters) are a third, non-differentiable output, or `deterministic`: handed to
    projective_icp_backward_batch, None = the environment at backward time), then points and normals of every sequence's map.  Gradients reach vertex, init_poses and the map points /
    normals that require grad (needs_input_grad decides which outputs the kernel is asked for); the association is hard
    and a constant, as are depth, K, model_poses and the live normals.  The backward re-reads the map rows, so the map
    buffers must hold at backward time what they held at the forward; in-place steps write through raw pointers, which
    torch's version counters do not see, so a caller that can tell passes `guard`, a callable that raises when the map
    has changed (ProjectiveICPOdometryProvider does).  Returns (poses (B, 4, 4), trace (B, numiters, 8), not
    differentiable)."""

    @staticmethod
    def forward(ctx, vertex, normal, depth, K, index, model_poses, init_poses, cfg, *flat):
        return _picp_taped_forward(ctx, (vertex, normal, depth, K, index, model_poses, init_poses), cfg, flat)

    @staticmethod
    def backward(ctx, T_bar, *_constants_bar):
        return _picp_taped_backward(ctx, T_bar, weighted=False)


class WeightedProjectiveICPFunction(torch.autograd.Function):
    """ProjectiveICPFunction with per-pixel weights: forward = gs_projective_icp_weighted_batch_f32 with a tape, backward
    = one call of gs_projective_icp_weighted_backward_batch_f32.  Inputs: vertex, normal, depth, K, index, model_poses,
    init_poses, pixel_weights (B, H, W), cfg (as ProjectiveICPFunction's), then points and normals of every sequence's
    map.  Gradients reach what ProjectiveICPFunction's reach and pixel_weights (needs_input_grad decides whether the
    kernel is asked for it); which pixels are masked is a constant, like the association.  Returns as
    ProjectiveICPFunction."""

    @staticmethod
    def forward(ctx, vertex, normal, depth, K, index, model_poses, init_poses, pixel_weights, cfg, *flat):
        return _picp_taped_forward(ctx, (vertex, normal, depth, K, index, model_poses, init_poses, pixel_weights), cfg,
                                   flat)

    @staticmethod
    def backward(ctx, T_bar, *_constants_bar):
        return _picp_taped_backward(ctx, T_bar, weighted=True)


def projective_icp(vertex, normal, depth, K, index, model_pose, map_points, map_normals, init_pose, *, n_dev=None,
                   stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0, return_trace=False,
                   differentiable=False, huber_delta=0.0, huber_k=0.0, return_scale=False, deterministic=None,
                   pixel_weights=None):
    """projective_icp_batch for one sequence without the batch dimension: vertex / normal (H, W, 3), depth (H, W), K /
    model_pose / init_pose (4, 4), index (H, W) int64; n_dev: device int64[1] holding the actual row count of the map
    (map_points.shape[0] is then an upper bound).  Returns the pose (4, 4) (and the trace (numiters, 8)).
    differentiable, huber_delta, huber_k, return_scale (the thresholds (numiters,)), deterministic, pixel_weights
    ((H, W) float32): see projective_icp_batch."""
    _picp_deterministic("projective_icp", "deterministic", deterministic)
    if pixel_weights is not None:
        _picp_tensors("projective_icp", (("pixel_weights", pixel_weights),))
        pixel_weights = pixel_weights.unsqueeze(0)
    _picp_tensors("projective_icp", (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K), ("index", index),
                                     ("model_pose", model_pose), ("init_pose", init_pose)))
    r = projective_icp_batch(vertex.unsqueeze(0), normal.unsqueeze(0), depth.unsqueeze(0), K.reshape(1, 4, 4),
                             index.unsqueeze(0), model_pose.reshape(1, 4, 4), [(map_points, map_normals, None, n_dev)],
                             init_pose.reshape(1, 4, 4), stride=stride, numiters=numiters, damp=damp,
                             dist_thresh=dist_thresh, angle_thresh=angle_thresh, return_trace=return_trace,
                             differentiable=differentiable, huber_delta=huber_delta, huber_k=huber_k,
                             return_scale=return_scale, deterministic=deterministic, pixel_weights=pixel_weights)
    return tuple(x[0] for x in r) if isinstance(r, tuple) else r[0]


def projective_icp_rows(vertex, normal, depth, K, index, model_pose, map_points, map_normals, pose, *, n_dev=None,
                        stride=1, dist_thresh=0.1, angle_thresh=30.0, huber_delta=0.0, return_weights=False,
                        huber_k=0.0, pixel_weights=None):
    """ONE linearisation of the projective ICP at `pose` (gs_projective_icp_rows_f32), arguments as projective_icp.  With
    nslots = ceil(H / stride) * ceil(W / stride), slot i * ceil(W / stride) + j standing for pixel (i stride, j stride):
    ProjectiveRows(code int32 (nslots,): 0 used, 1 no depth, 2 outside the model view, 3 no (or a stale) winner, 4 too
    far, 5 normals disagree; row int64 (nslots,): the index image's entry where one was read (codes 0, 3, 4, 5), else -1;
    a (nslots, 6), b (nslots,): the point-to-plane row, zeros unless used; sums float64 (28,): 21 upper-triangular a_i
    a_j, 6 a_i b, b b; count int64 (1,)).
    huber_delta > 0 (gs_projective_icp_robust_rows_f32): sums are the Huber-weighted sums, a and b stay unweighted;
    return_weights=True returns (ProjectiveRows, weight float32 (nslots,): the weight of a used slot, 0 elsewhere).
    huber_k > 0 (gs_projective_icp_scaled_rows_f32): the threshold is max(huber_k * 1.4826 * the lower median of |b| over
    the used slots, huber_delta), derived at `pose`; return_weights=True then returns (ProjectiveRows, weight, threshold
    float32 (1,)).
    pixel_weights ((H, W) float32, see projective_icp_batch; gs_projective_icp_weighted_rows_f32): a masked slot has code
    6 and row -1; sums are the weighted sums; `weight` is the total weight of a used slot, its pixel weight times its
    Huber weight; the returned shapes are those of the call without pixel weights."""
    who = "projective_icp_rows"
    opt = _picp_options(who, geometry=(stride, 1, 1.0, dist_thresh, angle_thresh), huber_delta=huber_delta,
                        huber_k=huber_k, flags=("return_weights",), return_weights=return_weights)
    _picp_tensors(who, (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K), ("index", index),
                        ("model_pose", model_pose), ("pose", pose)))
    if pixel_weights is not None:
        _picp_tensors(who, (("pixel_weights", pixel_weights),))
    weights = _picp_pixel_weights(who, None if pixel_weights is None else pixel_weights.unsqueeze(0), depth.unsqueeze(0))
    export, sizer = _picp_route("rows", opt, weights=weights is not None, tables=return_weights)
    seqs, held, dev, _, H, W = _picp_seqs(who, vertex.unsqueeze(0), normal.unsqueeze(0), depth.unsqueeze(0),
                                          K.reshape(1, 4, 4), index.unsqueeze(0), model_pose.reshape(1, 4, 4),
                                          [(map_points, map_normals, None, n_dev)], pose.reshape(1, 4, 4))
    _picp_scratch(seqs, dev, sizer, H, W, stride)
    ns = _picp_nslots(H, W, stride)
    res = ProjectiveRows(torch.empty(ns, dtype=torch.int32, device=dev), torch.empty(ns, dtype=torch.int64, device=dev),
                         torch.empty((ns, 6), dtype=f32, device=dev), torch.empty(ns, dtype=f32, device=dev),
                         torch.empty(28, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int64, device=dev))
    if weights is not None:
        require_device(*weights, held[0])
    # the weights and, where the median rule runs, the threshold it derived follow the rows when asked for
    extra = ()
    if return_weights:
        extra = (torch.empty(ns, dtype=f32, device=dev),) + \
            ((torch.empty(1, dtype=f32, device=dev),) if opt.huber_k > 0 else ())
    weight, th = (extra + (None, None))[:2]
    L, st, gates = lib(), stream(dev), (H, W, int(stride), opt.dist_th, opt.dot_th)
    rows, sums = [ptr(t) for t in res[:4]], [ptr(t) for t in res[4:]]
    if export == "weighted_rows":
        status = L.gs_projective_icp_weighted_rows_f32(seqs, ptr(weights[0]), *gates, opt.huber_delta, opt.huber_k,
                                                       *rows, ptr(weight), *sums, ptr(th), st)
    elif export == "scaled_rows":
        status = L.gs_projective_icp_scaled_rows_f32(seqs, *gates, opt.huber_k, opt.huber_delta, *rows, ptr(weight),
                                                     *sums, ptr(th), st)
    elif export == "robust_rows":
        status = L.gs_projective_icp_robust_rows_f32(seqs, *gates, opt.huber_delta, *rows, ptr(weight), *sums, st)
    else:
        status = L.gs_projective_icp_rows_f32(seqs, *gates, *rows, *sums, st)
    check(status, "gs_projective_icp_%s_f32" % export)
    return (res,) + extra if return_weights else res


# ----------------------------------------------------------------------------------- projective ICP: the outlier mask
OutlierRule = collections.namedtuple("OutlierRule", ["hi", "lo", "floor", "min_support", "grow", "grow_depth"],
                                     defaults=(3.0, 1.5, 0.0, 6, 0, 0.02))
OutlierRule.__doc__ = """The validated parameters of the outlier mask (gs_picp_outliers.hip): a pixel is strong when its
residual exceeds hi * 1.4826 * median|b| (or the floor, metres) or one of the two gates rejected it, eligible from
lo * 1.4826 * median|b|; a strong pixel with min_support strong pixels in its 3 x 3 window is a seed; the seeds grow for
`grow` steps over eligible 4-neighbours whose depth differs by at most grow_depth metres.  The defaults are starting
points, not tuned to any sensor."""
OUTLIER_MAX_GROW = 16


def _outlier_region_args(who, min_support, grow, grow_depth):
    """the value checks of the region pass: (min_support, grow, grow_depth)"""
    for name, val, lo, hi in (("min_support", min_support, 1, 9), ("grow", grow, 0, OUTLIER_MAX_GROW)):
        if isinstance(val, bool) or not isinstance(val, int):
            raise TypeError("{}: {} must be of type int; but was of type {}.".format(who, name, type(val)))
        if not lo <= val <= hi:
            raise ValueError("{}: {} ({}) must be within {} ... {}.".format(who, name, val, lo, hi))
    return min_support, grow, _picp_number(who, "grow_depth", grow_depth)


def _outlier_rule(who, hi=3.0, lo=1.5, floor=0.0, min_support=6, grow=0, grow_depth=0.02):
    """Validates into an OutlierRule, in the order of its fields: hi >= lo > 0, floor >= 0 (all finite), min_support
    within 1 ... 9, grow within 0 ... 16, grow_depth >= 0"""
    hi, lo, floor = (_picp_number(who, name, val) for name, val in (("hi", hi), ("lo", lo), ("floor", floor)))
    if not lo > 0:
        raise ValueError("{}: lo ({}) must be positive.".format(who, lo))
    if not hi >= lo:
        raise ValueError("{}: hi ({}) must be at least lo ({}).".format(who, hi, lo))
    return OutlierRule(hi, lo, floor, *_outlier_region_args(who, min_support, grow, grow_depth))


def region_mask(classes, depth, *, min_support=6, grow=0, grow_depth=0.02):
    """The region pass of the outlier mask (gs_region_mask_u8: one launch, tiles with a halo in LDS, bit-exact) for any
    number of images: classes (..., H, W) uint8 (bit 0 strong, bit 1 eligible), depth (..., H, W) float32.  A strong
    pixel with at least min_support strong pixels in its 3 x 3 window (itself included, pixels outside the image not) is
    a seed; for `grow` steps the seeds spread to eligible 4-neighbours whose depth differs by at most grow_depth.
    Returns the mask (..., H, W) uint8 of 0 / 1."""
    who = "region_mask"
    _picp_tensors(who, (("classes", classes), ("depth", depth)))
    min_support, grow, grow_depth = _outlier_region_args(who, min_support, grow, grow_depth)
    if classes.dtype != torch.uint8:
        raise TypeError("{}: classes must be uint8; got {}".format(who, classes.dtype))
    if depth.dtype != f32:
        raise TypeError("{}: depth must be float32; got {}".format(who, depth.dtype))
    if classes.ndim < 2 or tuple(classes.shape) != tuple(depth.shape) or classes.numel() == 0:
        raise ValueError("{}: expected classes and depth of one shape (..., H, W) with at least one pixel; got {} and "
                         "{}".format(who, tuple(classes.shape), tuple(depth.shape)))
    H, W = (int(x) for x in classes.shape[-2:])
    if H * W >= 1 << 31:
        raise ValueError("{}: image too large ({} x {})".format(who, H, W))
    _warn_detached(who, depth)
    classes, depth = classes.contiguous(), depth.detach().contiguous()
    dev = require_device(classes, depth)
    mask = torch.empty(classes.shape, dtype=torch.uint8, device=dev)
    check(lib().gs_region_mask_u8(ptr(classes), ptr(depth), ptr(mask), classes.numel() // (H * W), H, W, min_support, grow,
                                  grow_depth, stream(dev)), "gs_region_mask_u8")
    return mask


def projective_icp_outliers_batch(vertex, normal, depth, K, index, model_poses, maps, poses, *, hi=3.0, lo=1.5, floor=0.0,
                                  min_support=6, grow=0, grow_depth=0.02, dist_thresh=0.1, angle_thresh=30.0,
                                  pixel_weights=None, return_classes=False, return_thresholds=False):
    """The outlier mask of B sequences at `poses` (B, 4, 4), inputs as projective_icp_batch: which pixels of the live
    frames the model view does not explain, as a (B, H, W) uint8 image of 0 / 1 -- at every pixel, whatever stride the
    solve ran with.  The rule (gs_picp_outliers.hip, tests/outlier_mask_ref.py; everything on the device, nothing read
    back, bit-exact): code and residual b of each pixel as projective_icp_rows(stride=1) gives them at the pose; med =
    the lower median of |b| over the used pixels; a pixel is STRONG when it is used and |b| > max(hi * 1.4826 * med,
    floor), or when a gate rejected it (too far, normals disagree), ELIGIBLE when strong or used with |b| > max(lo *
    1.4826 * med, floor); a strong pixel with at least min_support strong pixels in its 3 x 3 window is a seed, and the
    seeds grow for `grow` steps over eligible 4-neighbours whose depth differs by at most grow_depth metres (region_mask).
    Pixels without depth, outside the model view, without a winner or masked by pixel_weights are never in the mask.
    floor (metres) matters on data without noise, where the median is 0 and every residual would be an outlier.
    return_classes: also the class bytes (B, H, W) uint8 (bit 0 strong, bit 1 eligible); return_thresholds: also the
    two thresholds (B, 2) float32, last."""
    who = "projective_icp_outliers"
    weights = _picp_pixel_weights(who, pixel_weights, depth)
    dist_th, dot_th = _picp_args(1, 1, 1.0, dist_thresh, angle_thresh)
    rule = _outlier_rule(who, hi, lo, floor, min_support, grow, grow_depth)
    _picp_flag(who, "return_classes", return_classes)
    _picp_flag(who, "return_thresholds", return_thresholds)
    seqs, held, dev, Bn, H, W = _picp_seqs(who, vertex, normal, depth, K, index, model_poses, maps, poses)
    L, ws = lib(), Workspace.get(dev)
    nbytes = L.gs_picp_outlier_classes_scratch_bytes(H, W)
    for b, u in enumerate(seqs):
        u.scratch = ws.bytes("picp_outliers%d" % b, nbytes).data_ptr()
    wptrs = None
    if weights is not None:
        require_device(*weights, held[0])
        wptrs = _picp_weight_ptrs(weights)
    classes = torch.empty((Bn, H, W), dtype=torch.uint8, device=dev)
    th = torch.empty((Bn, 2), dtype=f32, device=dev) if return_thresholds else None
    cptrs = (_C.C.c_void_p * Bn)(*[classes.data_ptr() + b * H * W for b in range(Bn)])
    tptrs = None if th is None else (_C.C.c_void_p * Bn)(*[th.data_ptr() + b * 8 for b in range(Bn)])
    check(L.gs_picp_outlier_classes_batch_f32(seqs, wptrs, cptrs, tptrs, Bn, H, W, dist_th, dot_th, rule.hi, rule.lo,
                                              rule.floor, stream(dev)), "gs_picp_outlier_classes_batch_f32")
    mask = torch.empty((Bn, H, W), dtype=torch.uint8, device=dev)
    check(L.gs_region_mask_u8(ptr(classes), ptr(held[2]), ptr(mask), Bn, H, W, rule.min_support, rule.grow,
                              rule.grow_depth, stream(dev)), "gs_region_mask_u8")
    res = (mask,) + ((classes,) if return_classes else ()) + ((th,) if return_thresholds else ())
    return res if len(res) > 1 else mask


def projective_icp_outliers(vertex, normal, depth, K, index, model_pose, map_points, map_normals, pose, *, n_dev=None,
                            hi=3.0, lo=1.5, floor=0.0, min_support=6, grow=0, grow_depth=0.02, dist_thresh=0.1,
                            angle_thresh=30.0, pixel_weights=None, return_classes=False, return_thresholds=False):
    """projective_icp_outliers_batch for one sequence without the batch dimension (arguments as projective_icp_rows):
    the mask (H, W) uint8 (and the classes (H, W), the thresholds (2,))."""
    who = "projective_icp_outliers"
    _picp_tensors(who, (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K), ("index", index),
                        ("model_pose", model_pose), ("pose", pose)))
    if pixel_weights is not None:
        _picp_tensors(who, (("pixel_weights", pixel_weights),))
        pixel_weights = pixel_weights.unsqueeze(0)
    r = projective_icp_outliers_batch(vertex.unsqueeze(0), normal.unsqueeze(0), depth.unsqueeze(0), K.reshape(1, 4, 4),
                                      index.unsqueeze(0), model_pose.reshape(1, 4, 4),
                                      [(map_points, map_normals, None, n_dev)], pose.reshape(1, 4, 4), hi=hi, lo=lo,
                                      floor=floor, min_support=min_support, grow=grow, grow_depth=grow_depth,
                                      dist_thresh=dist_thresh, angle_thresh=angle_thresh, pixel_weights=pixel_weights,
                                      return_classes=return_classes, return_thresholds=return_thresholds)
    return tuple(x[0] for x in r) if isinstance(r, tuple) else r[0]


# ----------------------------------------------------------------------------------- projective ICP with a colour term
ProjectiveColorRows =collections.namedtuple("ProjectiveColorRows", ["code", "row", "a", "b", "ac", "bc", "colored",
                                                                     "sums", "count", "color_count"])
PICP_COLOR_TRACE = 9


def _picp_refuse_differentiable(differentiable):
    if not isinstance(differentiable, bool):
        raise TypeError("projective_icp_color: differentiable must be of type bool; but was of type {}.".format(
            type(differentiable)))
    if differentiable:
        raise ValueError("projective_icp_color: the colour term has no backward pass yet (differentiable=True is not "
                         "supported; use projective_icp_batch for a pose on the autograd tape)")


def model_intensity(color, index):
    """The intensity image of a model view for the colour term (gs_model_intensity_f32): color (..., H, W, 3) float32 and
    index (..., H, W) int64 as render_map / render_map_batch return them -> (..., H, W, 4) float32 = (I, gx, gy, ok):
    I = 0.299 R + 0.587 G + 0.114 B, central differences gx, gy, ok = 1 where the pixel and its four neighbours are
    inside the image and hold a surfel (index >= 0), else ok = gx = gy = 0.  Built once per localisation."""
    _picp_tensors("model_intensity", (("color", color), ("index", index)))
    if color.ndim < 3 or color.shape[-1] != 3 or tuple(index.shape) != tuple(color.shape[:-1]) or color.numel() == 0:
        raise ValueError("model_intensity: expected color (..., H, W, 3) and index (..., H, W); got {} and {}".format(
            tuple(color.shape), tuple(index.shape)))
    if color.dtype != f32 or index.dtype != torch.int64:
        raise ValueError("model_intensity: color must be float32 and index int64; got {} and {}".format(
            color.dtype, index.dtype))
    _warn_detached("model_intensity", color)
    color, index = _c(color.detach()), index.contiguous()
    dev = require_device(color, index)
    H, W = int(color.shape[-3]), int(color.shape[-2])
    out = torch.empty(tuple(color.shape[:-1]) + (4,), dtype=f32, device=dev)
    check(lib().gs_model_intensity_f32(ptr(color), ptr(index), color.numel() // (3 * H * W), H, W, ptr(out), stream(dev)),
          "gs_model_intensity_f32")
    return out


def _picp_color_seqs(who, seqs, held, Bn, H, W, color, model):
    """the colour descriptors on top of the plain ones (_picp_seqs; the scratch, sized for the colour solve, is in them):
    shape / dtype / device checks of the live colour and the model intensity"""
    for name, t, shape in (("color", color, (Bn, H, W, 3)), ("model_intensity", model, (Bn, H, W, 4))):
        if not torch.is_tensor(t):
            raise TypeError("{}: expected {} to be of type tensor; got {}".format(who, name, type(t)))
        if tuple(t.shape) != shape or t.dtype != f32:
            raise ValueError("{}: expected {} to be float32 of shape {}; got {} {}".format(who, name, shape, t.dtype,
                                                                                           tuple(t.shape)))
    _warn_detached(who, color, model)
    color, model = _c(color.detach()), _c(model.detach())
    require_device(color, model, held[0])
    held += [color, model]
    cseqs = (_C.PicpColorSeq * Bn)()
    for b in range(Bn):
        cseqs[b].base = seqs[b]
        cseqs[b].color = color.data_ptr() + b * H * W * 12
        cseqs[b].model_intensity = model.data_ptr() + b * H * W * 16
    return cseqs


def projective_icp_color_batch(vertex, normal, depth, K, index, model_poses, maps, init_poses, color, model, *,
                               color_weight, stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0,
                               return_trace=False, out=None, differentiable=False, huber_delta=0.0,
                               color_huber_delta=0.0, huber_k=0.0, return_scale=False, color_huber_k=0.0,
                               return_color_scale=False, pixel_weights=None):
    """projective_icp_batch with a photometric term (gs_projective_icp_color_batch_f32: the same two launches per
    iteration for 8 sequences, nothing read back).  The arguments of projective_icp_batch, then color (B, H, W, 3): the
    live frames' colour, and model (B, H, W, 4): model_intensity of the views' rendered colour and index images.  A slot
    that passes the geometric gates and lands on a pixel with an intensity gradient (ok = 1) adds the row
    color_weight * (luma(color) - first-order model intensity at its projection) to the normal equations, next to its
    point-to-plane row.  color_weight: metres per intensity unit, finite and >= 0 (0 leaves the geometric solve).  Returns
    the poses (B, 4, 4), detached; with return_trace also (B, numiters, 9) rows [inliers, joint sum of squared residuals,
    xi(6), colour rows].  An iteration without geometric inliers leaves the pose as it is.  differentiable=True is
    refused: the colour term has no backward pass.
    huber_delta (metres) / color_huber_delta (intensity units), 0 = off: Huber weights on the point-to-plane residual and
    on the colour residual before color_weight is applied (gs_projective_icp_color_robust_batch_f32); the trace's second
    column is then the weighted joint sum of squares.
    huber_k, return_scale: as in projective_icp_batch, for the GEOMETRIC threshold (gs_projective_icp_color_scaled_batch_f32:
    the median of |b|, huber_delta its floor); without color_huber_k, color_huber_delta stays a constant.
    color_huber_k (0 = off; 1.345 is the usual constant): the COLOUR threshold is estimated from the colour residuals, per
    sequence and per iteration: cdelta = max(color_huber_k * 1.4826 * median|r|, color_huber_delta), with the lower median
    of |r| -- the colour residual before color_weight is applied -- over the slots that have a colour row at the pose the
    iteration linearises at (gs_projective_icp_color_joint_scaled_batch_f32); color_huber_delta is then a floor.  The
    threshold is in the units of the residuals, so colours in 0 ... 1 and in 0 ... 255 need no different constant.  It
    needs color_weight > 0 and combines with huber_delta and huber_k freely: the same two extra launches per iteration
    whichever of the two thresholds are estimated.  An iteration without a colour row, or whose median is 0, has
    cdelta = color_huber_delta.
    return_color_scale=True: the colour thresholds (B, numiters) float32 come after everything else in the returned
    tuple (color_huber_k = 0: color_huber_delta in every entry).
    pixel_weights: as in projective_icp_batch (gs_projective_icp_color_weighted_batch_f32): a masked pixel has no colour
    row either, and the colour products carry the pixel weight times the colour Huber weight."""
    _picp_refuse_differentiable(differentiable)
    weights = _picp_pixel_weights("projective_icp_color", pixel_weights, depth)
    opt = _picp_options("projective_icp_color", flags=("return_scale", "return_color_scale"),
                        color_weight=color_weight, color_huber_k=color_huber_k,
                        return_color_scale=return_color_scale, huber_delta=huber_delta, huber_k=huber_k,
                        return_scale=return_scale, color_huber_delta=color_huber_delta,
                        geometry=(stride, numiters, damp, dist_thresh, angle_thresh))
    return _picp_solve(opt, vertex, normal, depth, K, index, model_poses, maps, init_poses, color=color, model=model,
                       out=out, weights=weights, return_trace=return_trace, return_scale=return_scale,
                       return_color_scale=return_color_scale)


def projective_icp_color(vertex, normal, depth, K, index, model_pose, map_points, map_normals, init_pose, color, model,
                         *, color_weight, n_dev=None, stride=1, numiters=10, damp=1e-8, dist_thresh=0.1,
                         angle_thresh=30.0, return_trace=False, differentiable=False, huber_delta=0.0,
                         color_huber_delta=0.0, huber_k=0.0, return_scale=False, color_huber_k=0.0,
                         return_color_scale=False, pixel_weights=None):
    """projective_icp_color_batch for one sequence without the batch dimension (arguments as projective_icp, then color
    (H, W, 3) and model (H, W, 4)).  Returns the pose (4, 4) (and the trace (numiters, 9)).  huber_delta,
    color_huber_delta, huber_k, return_scale, color_huber_k, return_color_scale (the thresholds (numiters,)),
    pixel_weights ((H, W) float32): see projective_icp_color_batch."""
    if pixel_weights is not None:
        _picp_tensors("projective_icp_color", (("pixel_weights", pixel_weights),))
        pixel_weights = pixel_weights.unsqueeze(0)
    _picp_tensors("projective_icp_color", (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K),
                                           ("index", index), ("model_pose", model_pose), ("init_pose", init_pose),
                                           ("color", color), ("model_intensity", model)))
    r = projective_icp_color_batch(vertex.unsqueeze(0), normal.unsqueeze(0), depth.unsqueeze(0), K.reshape(1, 4, 4),
                                   index.unsqueeze(0), model_pose.reshape(1, 4, 4),
                                   [(map_points, map_normals, None, n_dev)], init_pose.reshape(1, 4, 4),
                                   color.unsqueeze(0), model.unsqueeze(0), color_weight=color_weight, stride=stride,
                                   numiters=numiters, damp=damp, dist_thresh=dist_thresh, angle_thresh=angle_thresh,
                                   return_trace=return_trace, differentiable=differentiable, huber_delta=huber_delta,
                                   color_huber_delta=color_huber_delta, huber_k=huber_k, return_scale=return_scale,
                                   color_huber_k=color_huber_k, return_color_scale=return_color_scale,
                                   pixel_weights=pixel_weights)
    return tuple(x[0] for x in r) if isinstance(r, tuple) else r[0]


def projective_icp_color_rows(vertex, normal, depth, K, index, model_pose, map_points, map_normals, pose, color, model,
                              *, color_weight, n_dev=None, stride=1, dist_thresh=0.1, angle_thresh=30.0, huber_delta=0.0,
                              color_huber_delta=0.0, return_weights=False, huber_k=0.0, color_huber_k=0.0,
                              pixel_weights=None):
    """ONE joint linearisation at `pose` (gs_projective_icp_color_rows_f32), arguments as projective_icp_color.
    ProjectiveColorRows: code, row, a, b as projective_icp_rows; ac (nslots, 6), bc (nslots,): the colour row, zeros
    unless colored; colored int32 (nslots,): 1 where the slot is used and its model pixel has ok = 1; sums float64 (28,):
    the joint sums; count, color_count int64 (1,).
    huber_delta / color_huber_delta > 0 (gs_projective_icp_color_robust_rows_f32): sums are the Huber-weighted joint sums,
    the rows stay unweighted; return_weights=True returns (ProjectiveColorRows, weight, color_weight) float32 (nslots,):
    the weight of a used slot and of a colour row, 0 elsewhere.
    huber_k / color_huber_k > 0 (gs_projective_icp_color_joint_scaled_rows_f32): the geometric / the colour threshold is
    derived at `pose` from the median of |b| over the used slots / of the colour residual |r| over the slots with a colour
    row, huber_delta / color_huber_delta its floor (see projective_icp_color_batch); return_weights=True then returns
    (ProjectiveColorRows, weight, color_weight, delta, cdelta): the two thresholds of this linearisation, float32 (1,)
    each (the constant where its rule is off).
    pixel_weights ((H, W) float32, gs_projective_icp_color_weighted_rows_f32): as in projective_icp_rows; the two weight
    tables hold the total weights (pixel weight times Huber weight); the returned shapes are those of the call without."""
    who = "projective_icp_color_rows"
    opt = _picp_options(who, flags=("return_weights",), color_weight=color_weight, huber_k=huber_k,
                        color_huber_k=color_huber_k, huber_delta=huber_delta, color_huber_delta=color_huber_delta,
                        return_weights=return_weights,
                        geometry=(stride, 1, 1.0, dist_thresh, angle_thresh))
    _picp_tensors(who, (("vertex", vertex), ("normal", normal), ("depth", depth), ("K", K), ("index", index),
                        ("model_pose", model_pose), ("pose", pose), ("color", color), ("model_intensity", model)))
    if pixel_weights is not None:
        _picp_tensors(who, (("pixel_weights", pixel_weights),))
    weights = _picp_pixel_weights(who, None if pixel_weights is None else pixel_weights.unsqueeze(0), depth.unsqueeze(0))
    export, sizer = _picp_route("color_rows", opt, weights=weights is not None, tables=return_weights)
    seqs, held, dev, _, H, W = _picp_seqs(who, vertex.unsqueeze(0), normal.unsqueeze(0), depth.unsqueeze(0),
                                          K.reshape(1, 4, 4), index.unsqueeze(0), model_pose.reshape(1, 4, 4),
                                          [(map_points, map_normals, None, n_dev)], pose.reshape(1, 4, 4))
    _picp_scratch(seqs, dev, sizer, H, W, stride)
    cseqs = _picp_color_seqs(who, seqs, held, 1, H, W, color.unsqueeze(0), model.unsqueeze(0))
    ns = _picp_nslots(H, W, stride)
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
    res = ProjectiveColorRows(e(ns, torch.int32), e(ns, torch.int64), e((ns, 6), f32), e(ns, f32), e((ns, 6), f32),
                              e(ns, f32), e(ns, torch.int32), e(28, torch.float64), e(1, torch.int64), e(1, torch.int64))
    if weights is not None:
        require_device(*weights, held[0])
    delta, k, cdelta, ck = opt.huber_delta, opt.huber_k, opt.color_huber_delta, opt.color_huber_k
    # the two weight tables and, where a median rule runs, the two thresholds follow the rows when asked for (a
    # threshold whose rule is off is the constant: the library writes the estimated ones only)
    extra = ()
    if return_weights:
        extra = (e(ns, f32), e(ns, f32)) + ((torch.full((1,), delta, dtype=f32, device=dev),
                                             torch.full((1,), cdelta, dtype=f32, device=dev)) if k > 0 or ck > 0 else ())
    wt, wtc, th, cth = (ptr(t) for t in (extra + (None,) * 4)[:4])
    L, st, gates = lib(), stream(dev), (H, W, int(stride), opt.dist_th, opt.dot_th, opt.color_weight)
    rows, sums = [ptr(t) for t in res[:7]], [ptr(t) for t in res[7:]]
    if export == "color_weighted_rows":
        status = L.gs_projective_icp_color_weighted_rows_f32(cseqs, ptr(weights[0]), *gates, delta, k, cdelta, ck, *rows,
                                                             wt, wtc, *sums, th, cth, st)
    elif export == "color_joint_scaled_rows":
        status = L.gs_projective_icp_color_joint_scaled_rows_f32(cseqs, *gates, k, delta, ck, cdelta, *rows, wt, wtc,
                                                                 *sums, th, cth, st)
    elif export == "color_robust_rows":
        status = L.gs_projective_icp_color_robust_rows_f32(cseqs, *gates, delta, cdelta, *rows, wt, wtc, *sums, st)
    else:
        status = L.gs_projective_icp_color_rows_f32(cseqs, *gates, *rows, *sums, st)
    check(status, "gs_projective_icp_%s_f32" % export)
    return (res,) + extra if return_weights else res


# ----------------------------------------------------------------------------------- pruning the map
PrunedMaps = collections.namedtuple("PrunedMaps", ["maps", "counts", "removed"])
PRUNE_MAX_MARKS = 64


def prune_map_batch(maps, min_confidence=None, keep=None, marks=None, young_mark=-1, out=None):
    """Stable compaction of the maps of B sequences into NEW buffers (gs_prune_map_dc_f32: count, tile scan, scatter and
    marks launch per 8 sequences; nothing is read back).  maps: per sequence a MapRows; normals / colors / features may
    be None.  With n = min(n_dev[0], n_bound), row r < n survives iff (keep is None or keep[r] != 0) and
    (min_confidence is None or r >= young_from or features[r, 0] >= min_confidence); min_confidence needs F == 1 (the
    confidence count)..  keep: per sequence a (rows,) bool / uint8 tensor or None..  marks: per sequence a device int64
    tensor of at most 64 ascending row indices or None; young_from = marks[b][young_mark] (young_mark, an int or one int
    per sequence; -1: every row is old enough), and the call REWRITES each mark as the number of survivors in front of
    it..  out: per sequence the four destination tensors (None where the source is None), at least n_bound rows each;
    default: new tensors of the sources' shapes (same capacity)..  Returns PrunedMaps(maps = per sequence (points,
    normals, colors, features), counts (B,) int64 on the device, removed (B,) int64 on the device); destination rows at
    or beyond the new count are not written."""
    Bn = len(maps)
    if Bn == 0:
        raise ValueError("prune_map: no maps")
    for name, val in (("keep", keep), ("marks", marks), ("out", out)):
        if val is not None and len(val) != Bn:
            raise ValueError("prune_map: %s must have one entry per map (%d), got %d" % (name, Bn, len(val)))
    young = [int(young_mark)] * Bn if not isinstance(young_mark, (list, tuple)) else [int(y) for y in young_mark]
    if len(young) != Bn:
        raise ValueError("prune_map: young_mark must be an int or one int per map")
    _warn_detached("prune_map", *[t for m in maps for t in m[:4]])
    held = [_map_rows(m) for m in maps]
    dev = require_device(*[t for h in held for t in h[:4]])
    if dev is None or held[0][0] is None:
        raise ValueError("prune_map: a map without points")
    ws = Workspace.get(dev)
    L = lib()
    seqs = (_C.PruneSeq * Bn)()
    cnt = torch.empty((2, Bn), dtype=torch.int64, device=dev)
    c0 = cnt.data_ptr()
    res, alive = [], []
    for b in range(Bn):
        P, N, Cc, F, n_bound, n_dev = held[b]
        if P is None or P.ndim != 2 or P.shape[1] != 3:
            raise ValueError("prune_map: points must be (rows, 3)")
        if any(t is not None and (t.ndim != 2 or t.shape[0] < P.shape[0]) for t in (N, Cc, F)) or \
                any(t is not None and t.shape[1] != 3 for t in (N, Cc)):
            raise ValueError("prune_map: normals / colors must be (rows, 3), features (rows, F), with as many rows as points")
        if min_confidence is not None and (F is None or F.shape[1] != 1):
            raise ValueError("prune_map: min_confidence needs one feature channel (the confidence count)")
        if out is None:
            dst = tuple(None if t is None else torch.empty_like(t) for t in (P, N, Cc, F))
        else:
            dst = tuple(out[b])
            for s, d in zip((P, N, Cc, F), dst):
                if (s is None) != (d is None) or (d is not None and (
                        d.dtype != f32 or not d.is_contiguous() or d.ndim != 2 or d.shape[1] != s.shape[1])):
                    raise ValueError("prune_map: out must hold a contiguous float32 tensor of the source's width for "
                                     "every attribute the map has, and None elsewhere")
        require_device(*dst, n_dev)
        kp = None if keep is None else keep[b]
        if kp is not None:
            if kp.dtype not in (torch.bool, torch.uint8) or kp.ndim != 1 or kp.shape[0] < n_bound:
                raise ValueError("prune_map: keep must be a (rows,) bool / uint8 tensor of at least n_bound rows")
            kp = kp.contiguous()
            kp = kp.view(torch.uint8) if kp.dtype == torch.bool else kp
        mk = None if marks is None else marks[b]
        if mk is not None and (mk.dtype != torch.int64 or mk.ndim != 1 or not mk.is_contiguous()):
            raise ValueError("prune_map: marks must be contiguous 1-d int64 tensors")
        require_device(kp, mk, P)
        u = seqs[b]
        u.points, u.normals, u.colors, u.features = (0 if t is None else t.data_ptr() for t in (P, N, Cc, F))
        u.F = 0 if F is None else int(F.shape[1])
        u.n_bound, u.n_dev = n_bound, (0 if n_dev is None else n_dev.data_ptr())
        u.points_out, u.normals_out, u.colors_out, u.features_out = (0 if t is None else t.data_ptr() for t in dst)
        u.capacity_out = min(int(t.shape[0]) for t in dst if t is not None)
        u.keep = 0 if kp is None else kp.data_ptr()
        u.marks, u.n_marks = (0, 0) if mk is None or mk.numel() == 0 else (mk.data_ptr(), int(mk.numel()))
        u.young_mark = young[b]
        u.n_out, u.removed_out = c0 + 8 * b, c0 + 8 * (Bn + b)
        u.scratch = ws.bytes("prune%d" % b, L.gs_prune_scratch_bytes(n_bound)).data_ptr()
        res.append(dst)
        alive.append((kp, mk))
    check(L.gs_prune_map_dc_f32(seqs, Bn, 0.0 if min_confidence is None else float(min_confidence),
                                0 if min_confidence is None else 1, stream(dev)), "gs_prune_map_dc_f32")
    return PrunedMaps(res, cnt[0], cnt[1])


def prune_map(points, normals, colors, features, n_dev=None, min_confidence=None, keep=None, marks=None, young_mark=-1,
              out=None):
    """prune_map_batch for one map: returns PrunedMaps((points, normals, colors, features), count int64[1], removed
    int64[1]), both counts on the device."""
    r = prune_map_batch([(points, normals, colors, features, None, n_dev)], min_confidence=min_confidence,
                        keep=None if keep is None else [keep], marks=None if marks is None else [marks],
                        young_mark=young_mark, out=None if out is None else [out])
    return PrunedMaps(r.maps[0], r.counts, r.removed)


# ----------------------------------------------------------------------------------- free-space carving
FreeSpace = collections.namedtuple("FreeSpace", ["violations", "keep"])
CARVE_MAX_WINDOW = 3


def _carve_args(who, margin, window, min_views):
    """the checks the C entry repeats, made before anything is allocated; names the argument"""
    if isinstance(margin, bool) or not isinstance(margin, (float, int)):
        raise TypeError("%s: margin must be of type float or int; but was of type %s." % (who, type(margin)))
    for name, val in (("window", window), ("min_views", min_views)):
        if isinstance(val, bool) or not isinstance(val, int):
            raise TypeError("%s: %s must be of type int; but was of type %s." % (who, name, type(val)))
    margin = float(margin)
    if not (margin >= 0.0 and margin != float("inf")):
        raise ValueError("%s: margin must be finite and >= 0; got %r" % (who, margin))
    if not 0 <= window <= CARVE_MAX_WINDOW:
        raise ValueError("%s: window must be in 0..%d; got %r" % (who, CARVE_MAX_WINDOW, window))
    if min_views < 1:
        raise ValueError("%s: min_views must be >= 1; got %r" % (who, min_views))
    return margin, int(window), int(min_views)


def free_space_batch(maps, depth, poses, K, *, margin=0.05, window=1, min_views=1, out=None):
    """Which rows of B maps do L depth frames each see through (gs_free_space_dc_f32: one launch per 8 sequences,
    whatever L is; nothing is read back).  maps: per sequence a MapRows, the full form only: points and the counts are
    read.  depth (B, L, H, W) or (B, L, H, W, 1), poses (B, L, 4, 4) camera-to-world, K (B, 4, 4).  A row violates a
    view iff it projects into the frame (the projection of the map update and of render_map), its pixel has depth > 0
    and every pixel with depth > 0 of the (2 window + 1)^2 square around it, clipped to the image, has (depth - z) >
    margin in float32 (z: the row's camera-frame depth)..  Returns FreeSpace(violations, keep): per sequence an (n_bound,)
    int32 tensor (views the row violates) and an (n_bound,) uint8 tensor (violations < min_views); rows at or beyond the
    device count hold 0 in both..  out: a FreeSpace (or pair) of per-sequence lists to write into (a list, or an entry of
    it, may be None: that output is then not produced)..  The result is detached and never on the autograd tape: the mask
    is a constant, like the association."""
    who = "free_space"
    margin, window, min_views = _carve_args(who, margin, window, min_views)
    for name, val in (("depth", depth), ("poses", poses), ("K", K)):
        if not torch.is_tensor(val):
            raise TypeError("%s: expected %s to be of type tensor; got %s" % (who, name, type(val)))
    if not isinstance(maps, (list, tuple)) or len(maps) == 0:
        raise ValueError("%s: maps must be a non-empty list of (points, normals, colors, ccounts, n_bound, n_dev)" % who)
    Bn = len(maps)
    if depth.ndim == 5 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth.ndim != 4 or depth.shape[0] != Bn or depth.shape[1] == 0 or depth.shape[2] == 0 or depth.shape[3] == 0:
        raise ValueError("%s: depth must be (B, L, H, W) or (B, L, H, W, 1) with B = %d maps and L, H, W >= 1; got %s"
                         % (who, Bn, tuple(depth.shape)))
    Lv, H, W = (int(s) for s in depth.shape[1:])
    if tuple(poses.shape) != (Bn, Lv, 4, 4):
        raise ValueError("%s: poses must be %s; got %s" % (who, (Bn, Lv, 4, 4), tuple(poses.shape)))
    if tuple(K.shape) != (Bn, 4, 4):
        raise ValueError("%s: K must be %s; got %s" % (who, (Bn, 4, 4), tuple(K.shape)))
    if H * W >= 1 << 31:
        raise ValueError("%s: depth images of 2^31 pixels or more are not supported" % who)
    if out is not None and (len(out) != 2 or any(o is not None and len(o) != Bn for o in out)):
        raise ValueError("%s: out must be (violations, keep), each a list with one entry per map or None" % who)
    for b, m in enumerate(maps):
        if not isinstance(m, (list, tuple)) or len(m) != 6 or not torch.is_tensor(m[0]):
            raise ValueError("%s: maps[%d] must be (points, normals, colors, ccounts, n_bound, n_dev)" % (who, b))
        if m[0].ndim != 2 or m[0].shape[1] != 3:
            raise ValueError("%s: points must be (rows, 3); got %s for maps[%d]" % (who, tuple(m[0].shape), b))
    poses, K = _c(poses.detach()), _c(K.detach())
    # the images are read in place where their rows are contiguous (a frame slice of a longer stack keeps its strides)
    depth = depth.detach() if depth.dtype == f32 else depth.detach().to(f32)
    if depth.stride(3) != 1 or depth.stride(2) != W:
        depth = depth.contiguous()
    dev = require_device(poses, K, depth[0, 0])
    seqs = (_C.CarveSeq * Bn)()
    viol, keep, held = [], [], [_map_rows(m, read=("points",)) for m in maps]
    for b, m in enumerate(held):
        require_device(m.points, m.n_dev, poses)
        if m.n_bound < 0:
            raise ValueError("%s: negative n_bound" % who)
        outs = _seq_outs(who, out, (("violations", torch.int32), ("keep", torch.uint8)), b, m.n_bound, dev)
        require_device(outs[0], outs[1], poses)
        u = seqs[b]
        u.map = _map_view(m)
        if m.n_bound == 0:
            u.map.points = None   # (an empty map: nothing to read)
        u.depth = depth.data_ptr() + b * int(depth.stride(0)) * 4
        u.depth_stride_view = int(depth.stride(1)) if Lv > 1 else H * W
        u.poses16, u.K16 = poses.data_ptr() + b * Lv * 64, K.data_ptr() + b * 64
        u.violations, u.keep = (0 if t is None else t.data_ptr() for t in outs)
        viol.append(outs[0])
        keep.append(outs[1])
    check(lib().gs_free_space_dc_f32(seqs, Bn, Lv, H, W, margin, window, min_views, stream(dev)),
          "gs_free_space_dc_f32")
    return FreeSpace(viol, keep)


def free_space(points, depth, poses, K, *, n_dev=None, margin=0.05, window=1, min_views=1, out=None):
    """One map against L depth frames: free_space_batch for B = 1 without the batch dimension.  points (rows, 3); depth
    (L, H, W), (L, H, W, 1) or (H, W); poses (L, 4, 4) or (4, 4); K (4, 4); n_dev: device int64[1] holding the actual
    row count (points.shape[0] is then an upper bound).  Returns FreeSpace(violations (rows,) int32, keep (rows,)
    uint8)."""
    for name, val in (("points", points), ("depth", depth), ("poses", poses), ("K", K)):
        if not torch.is_tensor(val):
            raise TypeError("free_space: expected %s to be of type tensor; got %s" % (name, type(val)))
    if depth.ndim == 2:
        depth = depth.unsqueeze(0)
    if poses.ndim == 2:
        poses = poses.unsqueeze(0)
    if tuple(K.shape) != (4, 4):
        raise ValueError("free_space: K must be (4, 4); got %s" % (tuple(K.shape),))
    if out is not None:
        if len(out) != 2:
            raise ValueError("free_space: out must be (violations, keep)")
        out = tuple(None if t is None else [t] for t in out)
    r = free_space_batch([(points, None, None, None, None, n_dev)], depth.unsqueeze(0), poses.unsqueeze(0),
                         K.reshape(1, 4, 4), margin=margin, window=window, min_views=min_views, out=out)
    return FreeSpace(r.violations[0], r.keep[0])


# ----------------------------------------------------------------------------------- voxel thinning
VoxelKeep = collections.namedtuple("VoxelKeep", ["keep", "winner", "unplaced"])
VOXEL_MAX_ROWS = (1 << 31) - 1


def _voxel_args(who, voxel_size):
    """the check the C entry repeats, made before anything is allocated; names the argument.  Returns the float32 value
    of the voxel size as a Python float: the number the kernel divides by"""
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, (float, int)):
        raise TypeError("%s: voxel_size must be of type float or int; but was of type %s." % (who, type(voxel_size)))
    v = float(voxel_size)
    if not (v > 0.0 and v != float("inf")):
        raise ValueError("%s: voxel_size must be finite and > 0; got %r" % (who, voxel_size))
    v32 = float(torch.tensor(v, dtype=torch.float32))
    if not (v32 > 0.0 and v32 != float("inf")):
        raise ValueError("%s: voxel_size must be finite and > 0 as a float32; got %r" % (who, voxel_size))
    return v32


def voxel_keep_batch(maps, voxel_size, *, out=None):
    """Which rows of B maps are the one surfel their voxel keeps (gs_voxel_keep_dc_f32: an elect and a resolve launch per
    8 sequences over a hash table in scratch; nothing is read back).  maps: per sequence a MapRows, the full form only:
    the points, the confidence (features, when it has one channel) and the counts are read.  With n = min(n_dev[0],
    n_bound): the voxel of a row is floor(p / voxel_size) per component in float32; a row is griddable iff its point is
    finite and every voxel index lies in [-2^20, 2^20); among the griddable rows < n of a voxel the winner has the
    largest confidence (its float32 bit pattern when >= +0.0, else 0: NaN and negative values score 0), ties go to the
    lowest row..  Returns VoxelKeep(keep, winner, unplaced): per sequence an (n_bound,) uint8 tensor (1: the row is below
    the count and is not griddable or is its voxel's winner) and an (n_bound,) int64 tensor (the winner of the row's
    voxel; the row itself when not griddable; -1 at or beyond the count), and a (B,) int32 tensor on the device (rows
    the table could not place and that were kept: 0)..  out: a pair (keep, winner) of per-sequence lists to write into (a
    list, or an entry of it, may be None: that output is then not produced)..  The result is detached and never on the
    autograd tape: the mask is a constant, like the association."""
    who = "voxel_keep"
    voxel_size = _voxel_args(who, voxel_size)
    if not isinstance(maps, (list, tuple)) or len(maps) == 0:
        raise ValueError("%s: maps must be a non-empty list of (points, normals, colors, features, n_bound, n_dev)" % who)
    Bn = len(maps)
    if out is not None and (len(out) != 2 or any(o is not None and len(o) != Bn for o in out)):
        raise ValueError("%s: out must be (keep, winner), each a list with one entry per map or None" % who)
    for b, m in enumerate(maps):
        if not isinstance(m, (list, tuple)) or len(m) != 6 or not torch.is_tensor(m[0]):
            raise ValueError("%s: maps[%d] must be (points, normals, colors, features, n_bound, n_dev)" % (who, b))
        if m[0].ndim != 2 or m[0].shape[1] != 3:
            raise ValueError("%s: points must be (rows, 3); got %s for maps[%d]" % (who, tuple(m[0].shape), b))
        if m[3] is not None and (not torch.is_tensor(m[3]) or m[3].ndim != 2 or m[3].shape[0] < m[0].shape[0]):
            raise ValueError("%s: features must be (rows, F) with as many rows as points, for maps[%d]" % (who, b))
    _warn_detached(who, *[t for m in maps for t in (m[0], m[3])])
    # (the confidence competes only as a single channel: any other feature layout is not read)
    held = [_map_rows(m, read=("points", "features") if m[3] is not None and m[3].shape[1] == 1 else ("points",))
            for m in maps]
    dev = require_device(*[t for h in held for t in h[:4]])
    unplaced = torch.empty((Bn,), dtype=torch.int32, device=dev)
    ws = Workspace.get(dev)
    L = lib()
    seqs = (_C.VoxelKeepSeq * Bn)()
    keep, winner = [], []
    for b in range(Bn):
        P, _, _, Cf, n_bound, n_dev = held[b]
        require_device(P, Cf, n_dev)
        if n_bound < 0:
            raise ValueError("%s: negative n_bound" % who)
        if n_bound > VOXEL_MAX_ROWS:
            raise ValueError("%s: maps of 2^31 rows or more are not supported" % who)
        outs = _seq_outs(who, out, (("keep", torch.uint8), ("winner", torch.int64)), b, n_bound, dev)
        require_device(outs[0], outs[1], P)
        nbytes = int(L.gs_voxel_keep_scratch_bytes(n_bound))
        u = seqs[b]
        u.points = P.data_ptr() if n_bound > 0 else 0
        u.confidence = Cf.data_ptr() if Cf is not None and n_bound > 0 else 0
        u.n_bound, u.n_dev = n_bound, (0 if n_dev is None else n_dev.data_ptr())
        u.keep, u.winner = (0 if t is None else t.data_ptr() for t in outs)
        u.unplaced = unplaced.data_ptr() + 4 * b
        u.scratch, u.scratch_bytes = ws.bytes("voxel%d" % b, nbytes).data_ptr(), nbytes
        keep.append(outs[0])
        winner.append(outs[1])
    check(L.gs_voxel_keep_dc_f32(seqs, Bn, voxel_size, stream(dev)), "gs_voxel_keep_dc_f32")
    return VoxelKeep(keep, winner, unplaced)


def voxel_keep(points, voxel_size, confidence=None, n_dev=None):
    """One cloud: voxel_keep_batch for B = 1.  points (rows, 3); confidence (rows,) or (rows, 1) or None (every score is 0:
    the first row of a voxel wins); n_dev: device int64[1] holding the actual row count (points.shape[0] is then an upper
    bound).  Returns VoxelKeep(keep (rows,) uint8, winner (rows,) int64, unplaced int32[1])."""
    _voxel_args("voxel_keep", voxel_size)
    for name, val in (("points", points),) + ((("confidence", confidence),) if confidence is not None else ()):
        if not torch.is_tensor(val):
            raise TypeError("voxel_keep: expected %s to be of type tensor; got %s" % (name, type(val)))
    if confidence is not None:
        if confidence.ndim == 1:
            confidence = confidence.unsqueeze(1)
        if confidence.ndim != 2 or confidence.shape[1] != 1:
            raise ValueError("voxel_keep: confidence must be (rows,) or (rows, 1); got %s" % (tuple(confidence.shape),))
    r = voxel_keep_batch([(points, None, None, confidence, None, n_dev)], voxel_size)
    return VoxelKeep(r.keep[0], r.winner[0], r.unplaced)


# ----------------------------------------------------------------------------------- feature layers
FEATURE_MAX_CHANNELS = 4096
FEATURE_DTYPES = {torch.float32: _C.FEATURE_F32, torch.float16: _C.FEATURE_F16}
FusedFeatures = collections.namedtuple("FusedFeatures", ["row_of_pix", "counts"])
CompactedFeatures = collections.namedtuple("CompactedFeatures", ["layers", "counts"])


def _feature_layers(who, layers):
    """per sequence (emb (capacity, C), weight (capacity,)) -> (C, dtype) after the checks every layer pass makes"""
    if len(layers) == 0:
        raise ValueError("%s: no layers" % who)
    C, dtype = None, None
    for emb, weight in layers:
        if not torch.is_tensor(emb) or not torch.is_tensor(weight):
            raise TypeError("%s: a layer is (emb, weight), two tensors" % who)
        if emb.dtype not in FEATURE_DTYPES:
            raise ValueError("%s: emb must be float32 or float16; got %s" % (who, emb.dtype))
        if emb.ndim != 2 or not 1 <= emb.shape[1] <= FEATURE_MAX_CHANNELS:
            raise ValueError("%s: emb must be (capacity, C) with C in 1..%d; got %s"
                             % (who, FEATURE_MAX_CHANNELS, tuple(emb.shape)))
        if weight.dtype != f32 or weight.ndim != 1 or weight.shape[0] < emb.shape[0]:
            raise ValueError("%s: weight must be a float32 (capacity,) tensor with as many rows as emb" % who)
        if C is None:
            C, dtype = int(emb.shape[1]), emb.dtype
        elif (int(emb.shape[1]), emb.dtype) != (C, dtype):
            raise ValueError("%s: every layer of a batch has the same channels and dtype" % who)
    return C, dtype


def _feature_scratch(ws, sizes):
    """one region of gs_scratch_bytes(rows, pixels) bytes per sequence, carved from the workspace's "scratch" buffer"""
    L = lib()
    need = [int(L.gs_scratch_bytes(int(r), int(p))) for r, p in sizes]
    base = ws.bytes("scratch", sum(need)).data_ptr()
    offs, at = [], 0
    for n in need:
        offs.append(base + at)
        at += n
    return offs


def fuse_features_batch(layers, n_old, best_pix, depth, alpha, feat=None, valid=None):
    """Fuses per-pixel feature images into the feature layers of B sequences, in place, AFTER the map update of the
    frame and on its tables (gs_fuse_features_batch: count, tile scan, rows and one wide fuse launch per 8 sequences;
    nothing is read back).  layers: per sequence (emb (capacity, C) float32 | float16, weight (capacity,) float32).
    n_old: per sequence (n_old_bound, n_old_dev): the map count BEFORE the update (n_old_dev: a device int64[1] tensor or
    None when the bound is exact).  best_pix: (B, H * W) int32 as update_map_fusion_batch_ returns it, or None (every
    pixel with depth is appended).  depth, alpha: (B, H, W) float32.  feat: (B, H, W, C) of the layers' dtype, or None
    (no pixel is valid: the appended rows are created with zeros and weight 0).  valid: (B, H, W) or (B, H * W) bool /
    uint8, or None (every pixel).  Pixel p goes to row best_pix[p] when 0 <= best_pix[p] < n_old (merged with the colour
    fusion's weights: emb = (w emb + a feat) / (w + a), weight = w + a, a = alpha[p]), to row n_old + rank(p) when
    best_pix[p] < 0 and depth[p] > 0 (emb = feat, weight = a), and nowhere otherwise.  Returns FusedFeatures(row_of_pix
    (B, H * W) int32, -1 for none; counts (B,) int64 on the device, the map's own new counts)."""
    who = "fuse_features"
    C, dtype = _feature_layers(who, layers)
    Bn = len(layers)
    if not torch.is_tensor(depth) or depth.ndim != 3 or depth.shape[0] != Bn:
        raise ValueError("%s: depth must be (%d, H, W)" % (who, Bn))
    _, H, W = depth.shape
    P = H * W
    if not torch.is_tensor(alpha) or tuple(alpha.shape) != (Bn, H, W):
        raise ValueError("%s: alpha must be (%d, %d, %d); got %s" % (who, Bn, H, W, tuple(alpha.shape)))
    if len(n_old) != Bn:
        raise ValueError("%s: n_old must have one (bound, device count) per layer" % who)
    if best_pix is not None and (best_pix.dtype != torch.int32 or tuple(best_pix.shape) != (Bn, P)):
        raise ValueError("%s: best_pix must be an int32 tensor of shape (%d, %d)" % (who, Bn, P))
    if feat is not None:
        if not torch.is_tensor(feat) or tuple(feat.shape) != (Bn, H, W, C):
            raise ValueError("%s: feat must be (%d, %d, %d, %d); got %s"
                             % (who, Bn, H, W, C, tuple(feat.shape) if torch.is_tensor(feat) else type(feat)))
        if feat.dtype != dtype:
            raise ValueError("%s: feat must have the layer's dtype %s; got %s" % (who, dtype, feat.dtype))
        _warn_detached(who, feat)
        feat = feat.detach().contiguous()
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or \
                tuple(valid.shape) not in ((Bn, H, W), (Bn, P)):
            raise ValueError("%s: valid must be a bool / uint8 tensor of shape (%d, %d, %d) or (%d, %d)"
                             % (who, Bn, H, W, Bn, P))
        valid = valid.contiguous()
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    best_pix = None if best_pix is None else best_pix.contiguous()
    views = [_batch_view(depth, 2), _batch_view(alpha, 2)]
    dev = require_device(best_pix, feat, valid, *[t for l in layers for t in l], *[n[1] for n in n_old])
    if any(v[0].device != dev for v in views):   # (slices of a frame stack: contiguous per sequence, not as a whole)
        raise _C.HipExtensionError("gradslam_amd kernels run on the GPU only; all tensors on one device")
    rows = torch.empty((Bn, P), dtype=torch.int32, device=dev)
    cnt = torch.empty(Bn, dtype=torch.int64, device=dev)
    scratch = _feature_scratch(Workspace.get(dev), [(int(n[0]), P) for n in n_old])
    seqs = (_C.FeatureFuseSeq * Bn)()
    es = 4 if dtype == f32 else 2
    for b in range(Bn):
        emb, weight = layers[b]
        bound, n_dev = n_old[b]
        if n_dev is not None and (n_dev.dtype != torch.int64 or n_dev.numel() != 1):
            raise ValueError("%s: a device count is an int64 tensor of one element" % who)
        u = seqs[b]
        u.emb, u.weight, u.capacity = emb.data_ptr(), weight.data_ptr(), int(emb.shape[0])
        u.n_old_bound, u.n_old_dev = int(bound), (0 if n_dev is None else n_dev.data_ptr())
        u.best_pix = 0 if best_pix is None else best_pix.data_ptr() + 4 * P * b
        u.depth, u.alpha = (v[1] + b * v[2] for v in views)
        u.feat = 0 if feat is None else feat.data_ptr() + es * P * C * b
        u.valid = 0 if valid is None else valid.data_ptr() + P * b
        u.row_of_pix, u.n_out, u.scratch = rows.data_ptr() + 4 * P * b, cnt.data_ptr() + 8 * b, scratch[b]
    check(lib().gs_fuse_features_batch(seqs, Bn, H, W, C, FEATURE_DTYPES[dtype], stream(dev)), "gs_fuse_features_batch")
    return FusedFeatures(rows, cnt)


def compact_features_batch(layers, n, keep, out=None):
    """Stable compaction of the feature layers of B sequences into NEW buffers by a keep mask
    (gs_compact_features_batch: count, tile scan and scatter launch per 8 sequences; nothing is read back).  layers: per
    sequence (emb (rows, C), weight (rows,)).  n: per sequence (n_bound, n_dev) as in MapRows.  keep: per sequence a
    (rows,) bool / uint8 tensor of at least n_bound entries.  out: per sequence (emb_out, weight_out) with at least
    n_bound rows; default: new tensors of the sources' shapes.  Survivor k of the first min(n_dev[0], n_bound) rows
    becomes row k, bit for bit: with the same mask these are the rows prune_map_batch keeps.  Returns
    CompactedFeatures(layers = per sequence (emb, weight), counts (B,) int64 on the device); destination rows at or
    beyond the new count are not written."""
    who = "compact_features"
    C, dtype = _feature_layers(who, layers)
    Bn = len(layers)
    for name, val in (("n", n), ("keep", keep), ("out", out)):
        if val is not None and len(val) != Bn:
            raise ValueError("%s: %s must have one entry per layer (%d), got %d" % (who, name, Bn, len(val)))
    if out is None:
        out = [(torch.empty_like(e), torch.empty_like(w)) for e, w in layers]
    else:
        _feature_layers(who, out)
        if any(o[0].shape[1] != C or o[0].dtype != dtype for o in out):
            raise ValueError("%s: out must hold layers of the sources' channels and dtype" % who)
    bounds = [min(int(layers[b][0].shape[0]), int(n[b][0])) for b in range(Bn)]
    keeps = []
    for b in range(Bn):
        kp = keep[b]
        if not torch.is_tensor(kp) or kp.dtype not in (torch.bool, torch.uint8) or kp.ndim != 1 or kp.shape[0] < bounds[b]:
            raise ValueError("%s: keep must be a (rows,) bool / uint8 tensor of at least n_bound rows" % who)
        kp = kp.contiguous()
        keeps.append(kp.view(torch.uint8) if kp.dtype == torch.bool else kp)
    dev = require_device(*[t for l in layers for t in l], *[t for l in out for t in l], *[x[1] for x in n], *keeps)
    cnt = torch.empty(Bn, dtype=torch.int64, device=dev)
    scratch = _feature_scratch(Workspace.get(dev), [(r, 0) for r in bounds])
    seqs = (_C.FeatureCompactSeq * Bn)()
    for b in range(Bn):
        kp, n_dev = keeps[b], n[b][1]
        u = seqs[b]
        u.emb, u.weight = layers[b][0].data_ptr(), layers[b][1].data_ptr()
        u.n_bound, u.n_dev = bounds[b], (0 if n_dev is None else n_dev.data_ptr())
        u.keep = kp.data_ptr()
        u.emb_out, u.weight_out = out[b][0].data_ptr(), out[b][1].data_ptr()
        u.capacity_out = min(int(out[b][0].shape[0]), int(out[b][1].shape[0]))
        u.n_out, u.scratch = cnt.data_ptr() + 8 * b, scratch[b]
    check(lib().gs_compact_features_batch(seqs, Bn, C, FEATURE_DTYPES[dtype], stream(dev)), "gs_compact_features_batch")
    return CompactedFeatures([tuple(o) for o in out], cnt)


# ----------------------------------------------------------------------------------- bilateral depth filter
BILATERAL_MAX_RADIUS = 8


def _bilateral_args(radius, sigma_space, sigma_range):
    import math
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise TypeError("bilateral_depth: radius must be of type int; but was of type {}.".format(type(radius)))
    if not 0 <= radius <= BILATERAL_MAX_RADIUS:
        raise ValueError("bilateral_depth: radius ({}) must be 0 ... {}.".format(radius, BILATERAL_MAX_RADIUS))
    for name, val in (("sigma_space", sigma_space), ("sigma_range", sigma_range)):
        if isinstance(val, bool) or not isinstance(val, (float, int)):
            raise TypeError("bilateral_depth: {} must be of type float or int; but was of type {}.".format(name, type(val)))
        if not (math.isfinite(val) and val > 0):
            raise ValueError("bilateral_depth: {} ({}) must be finite and > 0.".format(name, val))
    return radius, float(sigma_space), float(sigma_range)


def _bilateral_frames(depth):
    """(..., H, W) float32 device tensor -> ((n, H, W) tensor whose rows are contiguous, read in place where the leading
    dimensions collapse to one stride -- a frame slice of a longer stack, a channels-first stack, a column crop -- and
    copied otherwise)."""
    if depth.dtype != f32:
        depth = depth.to(f32)
    H, W = depth.shape[-2:]
    if depth.numel() == 0:
        raise ValueError("bilateral_depth: empty depth of shape {}".format(tuple(depth.shape)))
    d3 = depth.reshape(-1, H, W)     # (a view whenever the strides allow it)
    if d3.stride(2) != 1 or d3.stride(1) < W or (d3.shape[0] > 1 and d3.stride(0) < (H - 1) * d3.stride(1) + W):
        d3 = d3.contiguous()
    return d3


def _bilateral_forward(depth, radius, sigma_space, sigma_range, out=None, want_wsum=False):
    if not depth.is_cuda:
        require_device(depth)      # (raises: no CPU fallback)
    d3 = _bilateral_frames(depth)
    n, H, W = d3.shape
    dev = d3.device
    shape = tuple(depth.shape)
    if out is None:
        out = torch.empty(shape, dtype=f32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != f32:
        raise ValueError("bilateral_depth: out must be a float32 tensor of shape {}".format(shape))
    wsum = torch.empty(shape, dtype=f32, device=dev) if want_wsum else None
    if require_device(out, wsum) != dev:
        raise _C.HipExtensionError("tensors live on different devices: %s vs %s" % (dev, out.device))
    check(lib().gs_bilateral_depth_f32(d3.data_ptr(), d3.stride(0) if n > 1 else H * d3.stride(1), d3.stride(1), n, H, W,
                                       radius, two_sigma_sq(sigma_space), two_sigma_sq(sigma_range), ptr(out), ptr(wsum),
                                       stream(dev)), "gs_bilateral_depth_f32")
    return out, wsum


class BilateralDepthFunction(torch.autograd.Function):
    """depth (..., H, W) -> (bilaterally filtered depth, normaliser W); differentiable w.r.t. depth
    (gs_bilateral_depth_backward_f32: a gather per input pixel in a fixed order, bitwise reproducible).  Which pixels are
    valid is a constant; W is returned for inspection and carries no gradient."""

    @staticmethod
    def forward(ctx, depth, radius, sigma_space, sigma_range):
        d = depth.detach()
        out, wsum = _bilateral_forward(d, radius, sigma_space, sigma_range, want_wsum=True)
        ctx.save_for_backward(d, out, wsum)
        ctx.mark_non_differentiable(wsum)
        ctx.prm = (radius, sigma_space, sigma_range)
        return out, wsum

    @staticmethod
    def backward(ctx, out_bar, _wsum_bar):
        if out_bar is None:
            return None, None, None, None
        depth, out, wsum = ctx.saved_tensors
        radius, sigma_space, sigma_range = ctx.prm
        d3 = _bilateral_frames(depth)
        n, H, W = d3.shape
        dev = d3.device
        out_bar = _c(out_bar)
        d_bar = torch.empty(tuple(depth.shape), dtype=f32, device=dev)
        require_device(out, wsum, out_bar, d_bar)
        check(lib().gs_bilateral_depth_backward_f32(d3.data_ptr(), d3.stride(0) if n > 1 else H * d3.stride(1),
                                                    d3.stride(1), ptr(out), ptr(wsum), ptr(out_bar), n, H, W, radius,
                                                    two_sigma_sq(sigma_space), two_sigma_sq(sigma_range), ptr(d_bar),
                                                    stream(dev)), "gs_bilateral_depth_backward_f32")
        return d_bar.to(depth.dtype), None, None, None


def bilateral_depth(depth, radius=3, sigma_space=2.0, sigma_range=0.03, out=None, return_wsum=False):
    """Bilateral filter of every (H, W) image of a (..., H, W) depth stack in one launch (gs_bilateral_depth_f32; the
    arithmetic is pinned operation by operation, include/gradslam_hip.h).  A pixel is valid when depth > 0; invalid
    pixels are copied through and never contribute, so the valid mask is unchanged.  radius 0 ... 8 (0: the input
    bits), sigma_space in pixels, sigma_range in the unit of the depth.  The stack is read in place when its rows are
    contiguous and its leading dimensions collapse to one stride.  out: optional contiguous float32 tensor of depth's
    shape (not depth itself).  return_wsum: also return the normaliser W per pixel (0 at invalid pixels).
    With depth.requires_grad the call goes on the autograd tape (BilateralDepthFunction); `out` is then refused."""
    radius, sigma_space, sigma_range = _bilateral_args(radius, sigma_space, sigma_range)
    if depth.ndim < 2:
        raise ValueError("bilateral_depth: depth must be (..., H, W), got shape {}".format(tuple(depth.shape)))
    if torch.is_grad_enabled() and depth.requires_grad:
        if out is not None:
            raise ValueError("bilateral_depth: `out` cannot be given for a depth that requires grad")
        res, wsum = BilateralDepthFunction.apply(depth, radius, sigma_space, sigma_range)
        return (res, wsum) if return_wsum else res
    res, wsum = _bilateral_forward(depth, radius, sigma_space, sigma_range, out=out, want_wsum=return_wsum)
    return (res, wsum) if return_wsum else res


def render_map_backward_batch(maps, poses, K, index, upstream, H, W, radius=0, want=(True, True, True, True, True),
                              radii=None, max_radius=3):
    """Reverse mode of render_map_batch for B sequences in ONE call of gs_render_map_backward_dc_f32 (8 sequences and 4
    views per launch).  maps: per sequence a MapRows or its short form, as given to the forward (points and normals
    are read; normals may be None when upstream[2] is); poses (B, L, 4, 4), K (B, 4, 4), index (B, L, H, W) int64: the
    index image of the forward; upstream: (depth_bar (B, L, H, W[, 1]), color_bar (B, L, H, W, 3), normal_bar (B, L, H,
    W, 3), confidence_bar (B, L, H, W[, 1])), any of them None (its terms are skipped)..  want: which of (points_bar,
    normals_bar, colors_bar, ccounts_bar, poses_bar) to compute..  Returns (per-sequence list of (points_bar (rows, 3),
    normals_bar (rows, 3), colors_bar (rows, 3), ccounts_bar (rows, 1)) with None where not wanted, poses_bar (B, L, 4,
    4) or None); rows = points.shape[0], rows at or beyond the count hold zeros.
    radii, max_radius: those of the forward (gs_render_map_radii_backward_dc_f32; `radius` must then be 0)."""
    radii = _render_radii("render_map_backward", maps, radii, radius, max_radius)
    poses, K, index = _c(poses.detach()), _c(K.detach()), _c(index, torch.int64)
    ups = [None if t is None else _c(t.detach()) for t in upstream]
    dev = require_device(poses, K, index, *ups)
    Bn, Lv = int(poses.shape[0]), int(poses.shape[1])
    H, W = int(H), int(W)
    if len(maps) != Bn or tuple(poses.shape[2:]) != (4, 4) or tuple(K.shape) != (Bn, 4, 4) or \
            tuple(index.shape) != (Bn, Lv, H, W) or Lv == 0:
        raise ValueError("render_map_backward: expected poses (B, L, 4, 4), K (B, 4, 4) and index (B, L, H, W) for B = %d "
                         "maps; got %s, %s and %s" % (len(maps), tuple(poses.shape), tuple(K.shape), tuple(index.shape)))
    for t, c in zip(ups, (1, 3, 3, 1)):
        if t is not None and t.numel() != Bn * Lv * H * W * c:
            raise ValueError("render_map_backward: an upstream image does not match (B, L, H, W, %d)" % c)
    T_bar = torch.empty((Bn, Lv, 4, 4), dtype=f32, device=dev) if want[4] else None
    L = lib()
    ws = Workspace.get(dev)
    seqs = (_C.RenderBackwardSeq * Bn)()
    P1 = Lv * H * W
    rows_out, held = [], [_map_rows(m, read=("points", "normals"), four_ok=True) for m in maps]
    for b, m in enumerate(held):
        P, N, n_bound = m.points, m.normals, m.n_bound
        require_device(P, N, m.n_dev, poses)
        rows = int(P.shape[0])
        if P.ndim != 2 or P.shape[1] != 3 or (N is not None and N.shape[0] < rows):
            raise ValueError("render_map_backward: points must be (rows, 3) and the normals must hold as many rows")
        if N is None and ups[2] is not None:
            raise ValueError("render_map_backward: normal_bar given but the map has no normals")
        outs = [_rows_bar(rows, c, n_bound, dev) if want[i] else None for i, c in enumerate((3, 3, 3, 1))]
        rows_out.append(tuple(outs))
        u = seqs[b]
        u.map = _map_view(m)
        u.poses16, u.K16, u.index = poses.data_ptr() + b * Lv * 64, K.data_ptr() + b * 64, index.data_ptr() + b * P1 * 8
        u.depth_bar, u.color_bar, u.normal_bar, u.confidence_bar = (
            None if t is None else t.data_ptr() + b * P1 * c * 4 for t, c in zip(ups, (1, 3, 3, 1)))
        u.points_bar, u.normals_bar, u.colors_bar, u.ccounts_bar = (None if t is None else t.data_ptr() for t in outs)
        if T_bar is not None:
            u.poses_bar = T_bar.data_ptr() + b * Lv * 64
            u.scratch = ws.bytes("render_bwd%d" % b, L.gs_render_backward_scratch_bytes(Lv, H, W, n_bound)).data_ptr()
    if radii is not None:
        rptr, rheld = _radii_pointers(radii, dev)
        check(L.gs_render_map_radii_backward_dc_f32(seqs, rptr, Bn, Lv, H, W, max_radius, stream(dev)),
              "gs_render_map_radii_backward_dc_f32")
        return rows_out, T_bar
    check(L.gs_render_map_backward_dc_f32(seqs, Bn, Lv, H, W, int(radius), stream(dev)), "gs_render_map_backward_dc_f32")
    return rows_out, T_bar


class RenderMapFunction(torch.autograd.Function):
    """The model view of ONE sequence on the autograd tape: forward = gs_render_map_dc_f32 (the plain render, which also
    yields the index image), backward = one call of gs_render_map_backward_dc_f32 (render_map_backward_batch).  The
    render is a hard z-buffer: the winner of every pixel and the min_confidence / cull_backfaces filters are constants
    (as the correspondences of FuseAppendFunction are); gradients flow through the winner's depth, colour, camera-frame
    normal and confidence to the map rows and to the poses.  K and the index image get none.  Images the loss does not
    use reach the kernel as NULL (their terms are skipped; no zero images are made up).  The backward re-projects the
    map rows, so the map buffers must hold at backward time what they held at the forward (run backward before the next
    in-place step); in-place steps write through raw pointers, which torch's version counters do not see, so a caller
    that can tell passes `guard`, a callable that raises when the map has changed (Pointclouds.render does).  radii,
    max_radius: the model view with per-surfel radii (the gs_render_map_radii_* entries); the radii get no gradient."""

    @staticmethod
    def forward(ctx, points, normals, colors, ccounts, poses, K, n_bound, n_dev, H, W, radius, min_confidence,
                cull_backfaces, guard=None, radii=None, max_radius=3):
        if poses.ndim != 3 or tuple(poses.shape[1:]) != (4, 4) or tuple(K.shape) != (4, 4):
            raise ValueError("render_map: expected poses (L, 4, 4) and K (4, 4) per map; got %s and %s"
                             % (tuple(poses.shape), tuple(K.shape)))
        r = render_map_batch([(points, normals, colors, ccounts, n_bound, n_dev)], poses.unsqueeze(0), K.unsqueeze(0),
                             H, W, radius=radius, min_confidence=min_confidence, cull_backfaces=cull_backfaces,
                             radii=None if radii is None else [radii], max_radius=max_radius)
        r = RenderedViews(*[None if t is None else t[0] for t in r])
        ctx.save_for_backward(points, normals, poses, K, r.index, n_dev, None if radii is None else radii.detach())
        ctx.geom = (H, W, radius, n_bound, max_radius)
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (points, normals, colors, ccounts))
        ctx.guard = guard
        ctx.set_materialize_grads(False)   # an image the loss does not use arrives as None, not as a zero image
        ctx.mark_non_differentiable(r.index)
        return tuple(r)

    @staticmethod
    def backward(ctx, depth_bar, color_bar, normal_bar, conf_bar, _index_bar):
        if ctx.guard is not None:
            ctx.guard()
        points, normals, poses, K, index, n_dev, radii = ctx.saved_tensors
        H, W, radius, n_bound, max_radius = ctx.geom
        need = ctx.needs_input_grad
        ups = (depth_bar, color_bar, normal_bar, conf_bar)
        if all(t is None for t in ups):
            return (None,) * 16
        want = tuple(bool(need[i]) and ctx.shapes[i] is not None for i in range(4)) + (bool(need[4]),)
        rows_out, T_bar = render_map_backward_batch([(points, normals, n_bound, n_dev)], poses.unsqueeze(0),
                                                    K.unsqueeze(0), index.unsqueeze(0),
                                                    [None if t is None else t.unsqueeze(0) for t in ups], H, W, radius,
                                                    want=want, radii=None if radii is None else [radii],
                                                    max_radius=max_radius)
        outs = [None if t is None else t.view(shape) for t, shape in zip(rows_out[0], ctx.shapes)]
        return (outs[0], outs[1], outs[2], outs[3], None if T_bar is None else T_bar[0]) + (None,) * 11


# ----------------------------------------------------------------------------------- K7 (autograd)
def icp_with_tape(src, tgt, tgt_normals, init=None, numiters=20, damp=1e-8, dist_thresh=None, lambda_max=2.0,
                  B=1.0, B2=1.0, nu=200.0, mode=1):
    """(grad)ICP forward that also records the tape gs_icp_backward_f32 needs.  Returns (T, idx, tape, prm)."""
    src, tgt, tn = _c(src), _c(tgt), _c(tgt_normals)
    dev = require_device(src, tgt, tn)
    init = torch.eye(4, dtype=f32, device=dev) if init is None else _c(init)
    require_device(init)
    ns, nt = src.shape[0], tgt.shape[0]
    prm = _C.IcpParams(int(mode), int(numiters), float(damp), _thresh(dist_thresh),
                       float(lambda_max), float(B), float(B2), float(nu))
    T = torch.empty((4, 4), dtype=f32, device=dev)
    idx = torch.empty(ns, dtype=torch.int64, device=dev)
    scratch = Workspace.get(dev).bytes("icp", lib().gs_icp_scratch_bytes(ns, nt))
    tape = torch.empty(lib().gs_icp_tape_bytes(ns, int(numiters)), dtype=torch.uint8, device=dev)
    check(lib().gs_icp_tape_f32(ptr(src), ns, ptr(tgt), ptr(tn), nt, ptr(init), None, prm, ptr(T), ptr(idx),
                                ptr(scratch), ptr(tape), stream(dev)), "gs_icp_tape_f32")
    return T, idx, tape, prm


def icp_backward(tape, prm, src, tgt, tgt_normals, init, T_bar, need=(True, True, True, True)):
    """dL/dT -> (dL/dsrc, dL/dtgt, dL/dnormals, dL/dinit); entries not needed are None."""
    src, tgt, tn, init, T_bar = _c(src), _c(tgt), _c(tgt_normals), _c(init), _c(T_bar)
    dev = require_device(tape, src, tgt, tn, init, T_bar)
    ns, nt = src.shape[0], tgt.shape[0]
    gs = torch.empty_like(src) if need[0] else None
    gt = torch.empty_like(tgt) if need[1] else None
    gn = torch.empty_like(tn) if need[2] else None
    gi = torch.empty((4, 4), dtype=f32, device=dev) if need[3] else None
    scratch = Workspace.get(dev).bytes("icp_bwd", lib().gs_icp_backward_scratch_bytes(ns, nt))
    check(lib().gs_icp_backward_f32(ptr(tape), ptr(src), ns, ptr(tgt), ptr(tn), nt, ptr(init), prm, ptr(T_bar),
                                    ptr(gs), ptr(gt), ptr(gn), ptr(gi), ptr(scratch), stream(dev)),
          "gs_icp_backward_f32")
    return gs, gt, gn, gi


class GradICPFunction(torch.autograd.Function):
    """point_to_plane_gradICP as a differentiable op: forward = gs_icp_tape_f32, backward =
    gs_icp_backward_f32 (hand-written reverse mode; no PyTorch ops on the tape)."""

    @staticmethod
    def forward(ctx, src, tgt, tgt_normals, init, numiters, damp, dist_thresh, lambda_max, B, B2, nu, mode=1):
        T, idx, tape, prm = icp_with_tape(src, tgt, tgt_normals, init, numiters, damp, dist_thresh, lambda_max, B, B2,
                                          nu, mode)
        ctx.save_for_backward(src, tgt, tgt_normals, init, tape)
        ctx.prm = prm
        ctx.mark_non_differentiable(idx)
        return T, idx

    @staticmethod
    def backward(ctx, T_bar, _idx_bar):
        src, tgt, tn, init, tape = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:4])
        gs, gt, gn, gi = icp_backward(tape, ctx.prm, src, tgt, tn, init, T_bar.contiguous(), need)
        return (gs, gt, gn, gi) + (None,) * 8


def grad_icp(src, tgt, tgt_normals, init=None, numiters=20, damp=1e-8, dist_thresh=None, lambda_max=2.0, B=1.0,
             B2=1.0, nu=200.0, mode=1):
    """Differentiable gradICP (mode 1) / hard-LM ICP (mode 0): (T (4,4), idx (Ns,)).  Uses the plain forward when
    nothing requires grad."""
    dev = src.device
    init = torch.eye(4, dtype=f32, device=dev) if init is None else init
    if torch.is_grad_enabled() and any(t.requires_grad for t in (src, tgt, tgt_normals, init)):
        return GradICPFunction.apply(src, tgt, tgt_normals, init, numiters, damp, dist_thresh, lambda_max, B, B2, nu,
                                     mode)
    return icp(src, tgt, tgt_normals, init=init, mode=mode, numiters=numiters, damp=damp, dist_thresh=dist_thresh,
               lambda_max=lambda_max, B=B, B2=B2, nu=nu)


class FuseAppendFunction(torch.autograd.Function):
    """fuse_with_map of one sequence as a differentiable op (out of place): old map rows + frame maps -> fused map.
    forward = gs_fuse_append_f32 on a copy, backward = gs_fuse_append_backward_f32.  Correspondences (best_pix)
    and depth (validity only) are constants."""

    @staticmethod
    def forward(ctx, points, normals, colors, ccounts, gvertex, gnormal, rgb, alpha, depth, best_pix, renorm_all):
        n0 = points.shape[0]
        H, W = depth.shape[:2]
        dev = gvertex.device
        bufs = [torch.empty((n0 + H * W, c), dtype=f32, device=dev) for c in (3, 3, 3, 1)]
        for dst, src in zip(bufs, (points, normals, colors, ccounts)):
            dst[:n0] = src
        n1 = fuse_append_(*bufs, n0, best_pix, gvertex, gnormal, rgb, alpha, depth, renorm_all)
        ctx.save_for_backward(points, normals, colors, ccounts, gvertex, gnormal, rgb, alpha, depth, best_pix)
        ctx.renorm_all, ctx.n1 = int(renorm_all), n1
        return tuple(b[:n1] for b in bufs)

    @staticmethod
    def backward(ctx, P_bar, N_bar, C_bar, F_bar):
        points, normals, colors, ccounts, gvertex, gnormal, rgb, alpha, depth, best_pix = ctx.saved_tensors
        dev = gvertex.device
        n0, n1 = points.shape[0], ctx.n1
        H, W = depth.shape[:2]
        bars = [_c(t) if t is not None else torch.zeros((n1, c), dtype=f32, device=dev)
                for t, c in zip((P_bar, N_bar, C_bar, F_bar), (3, 3, 3, 1))]
        old = [torch.empty((n0, c), dtype=f32, device=dev) for c in (3, 3, 3, 1)]
        gv_b, gn_b, rgb_b = (torch.empty((H, W, 3), dtype=f32, device=dev) for _ in range(3))
        a_b = torch.empty((H, W), dtype=f32, device=dev)
        ws = Workspace.get(dev)
        check(lib().gs_fuse_append_backward_f32(ptr(_c(points)), ptr(_c(normals)), ptr(_c(colors)), ptr(_c(ccounts)), n0,
                                                ptr(best_pix), ptr(_c(gvertex)), ptr(_c(gnormal)), ptr(_c(rgb)),
                                                ptr(_c(alpha)), ptr(_c(depth)), H, W, int(ctx.renorm_all),
                                                ptr(bars[0]), ptr(bars[1]), ptr(bars[2]), ptr(bars[3]), n1, ptr(old[0]),
                                                ptr(old[1]), ptr(old[2]), ptr(old[3]), ptr(gv_b), ptr(gn_b), ptr(rgb_b),
                                                ptr(a_b), ptr(ws.scratch(n0, H * W)), stream(dev)),
              "gs_fuse_append_backward_f32")
        return old[0], old[1], old[2], old[3], gv_b, gn_b, rgb_b, a_b, None, None, None


class FrameMapsFunction(torch.autograd.Function):
    """depth (H,W) -> (vertex, normal, alpha); differentiable w.r.t. depth (gs_frame_maps_backward_f32)."""

    @staticmethod
    def forward(ctx, depth, K, sigma):
        v, n, a, _ = frame_maps(depth, K, sigma, want_valid=False)
        ctx.save_for_backward(depth, K)
        ctx.sigma = sigma
        return v, n, a

    @staticmethod
    def backward(ctx, v_bar, n_bar, a_bar):
        depth, K = ctx.saved_tensors
        depth_c, K_c = _c(depth), _c(K)
        dev = require_device(depth_c, K_c)
        H, W = depth_c.shape
        v_bar, n_bar, a_bar = _c(v_bar), _c(n_bar), _c(a_bar)
        d_bar = torch.empty((H, W), dtype=f32, device=dev) if ctx.needs_input_grad[0] else None
        scratch = torch.empty((H, W, 6), dtype=f32, device=dev) if n_bar is not None else None
        K_bar, k_scratch = None, None
        if ctx.needs_input_grad[1]:   # gradient w.r.t. the intrinsics (fx, fy, cx, cy entries)
            K_bar = torch.empty((4, 4), dtype=f32, device=dev)
            k_scratch = Workspace.get(dev).bytes("kbar", lib().gs_frame_maps_backward_kbar_scratch_bytes(H, W))
        check(lib().gs_frame_maps_backward_f32(ptr(depth_c), ptr(K_c), H, W, two_sigma_sq(ctx.sigma), ptr(v_bar),
                                               ptr(n_bar), ptr(a_bar), ptr(d_bar), ptr(scratch), ptr(K_bar),
                                               ptr(k_scratch), stream(dev)), "gs_frame_maps_backward_f32")
        return d_bar, K_bar, None


class GlobalMapsFunction(torch.autograd.Function):
    """(vertex, normal) + pose -> (gvertex, gnormal); differentiable w.r.t. the local maps and the pose."""

    @staticmethod
    def forward(ctx, vertex, normal, depth, pose):
        gv, gn = global_maps(vertex, normal, depth, pose)
        ctx.save_for_backward(depth, pose, vertex, normal)
        return gv, gn

    @staticmethod
    def backward(ctx, gv_bar, gn_bar):
        depth, pose, vertex, normal = ctx.saved_tensors
        depth_c, pose_c = _c(depth), _c(pose)
        dev = require_device(depth_c, pose_c)
        H, W = depth_c.shape[:2]
        gv_bar, gn_bar = _c(gv_bar), _c(gn_bar)
        v_bar = torch.empty((H, W, 3), dtype=f32, device=dev) if gv_bar is not None else None
        n_bar = torch.empty((H, W, 3), dtype=f32, device=dev) if gn_bar is not None else None
        check(lib().gs_global_maps_backward_f32(ptr(gv_bar), ptr(gn_bar), ptr(depth_c), ptr(pose_c), H, W, ptr(v_bar),
                                                ptr(n_bar), stream(dev)), "gs_global_maps_backward_f32")
        pose_bar = None
        if ctx.needs_input_grad[3]:
            pose_bar = torch.empty((4, 4), dtype=f32, device=dev)
            scratch = Workspace.get(dev).bytes("pose_bar", lib().gs_global_maps_pose_backward_scratch_bytes(H, W))
            check(lib().gs_global_maps_pose_backward_f32(ptr(_c(vertex)), ptr(_c(normal)), ptr(depth_c), ptr(gv_bar),
                                                         ptr(gn_bar), H, W, ptr(pose_bar), ptr(scratch), stream(dev)),
                  "gs_global_maps_pose_backward_f32")
        return v_bar, n_bar, None, pose_bar


class DownsampleFramePointsFunction(torch.autograd.Function):
    """global vertex map -> compact lattice points; backward scatters the adjoints to their pixels."""

    @staticmethod
    def forward(ctx, gvertex, depth, ds):
        pts, _, _ = downsample_frame(gvertex, None, None, depth, ds)
        ctx.save_for_backward(depth)
        ctx.ds = ds
        return pts

    @staticmethod
    def backward(ctx, pts_bar):
        (depth,) = ctx.saved_tensors
        depth_c, pts_bar = _c(depth), _c(pts_bar)
        dev = require_device(depth_c, pts_bar)
        H, W = depth_c.shape[:2]
        gv_bar = torch.empty((H, W, 3), dtype=f32, device=dev)
        ws = Workspace.get(dev)
        check(lib().gs_downsample_frame_backward_f32(ptr(pts_bar), ptr(depth_c), H, W, ctx.ds, ptr(gv_bar),
                                                     ptr(ws.scratch(0, H * W)), stream(dev)),
              "gs_downsample_frame_backward_f32")
        return gv_bar, None, None
