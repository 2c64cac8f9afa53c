"""Oracle for the backward pass of the frame maps (structures/rgbdimages.py:643-743 + slam/fusionutils.py:69-72):
float64 numpy reverse mode of depth -> (vertex, normal, alpha), pinned against the reference's own autograd
(tests/golden/depth_grad.npz: maps_depth_grad).  Test infrastructure only.

forward:  V[h,w] = ray[h,w] * depth * valid,  ray = (k00 w + k02, k11 h + k12, 1)
          dh[h,w] = V[h,w0+1] - V[h,w0], w0 = min(w, W-2);  dv[h,w] = V[h0+1,w] - V[h0,w], h0 = min(h, H-2)
          n = dh x dv;  N = n / where(|n| == 0, 1, |n|) * valid
          alpha = clamp(exp(-|V|^2 / (2 sigma^2)), 1e-7, 1.01)"""
import numpy as np


def frame_maps_backward(depth, K, sigma, v_bar, n_bar, a_bar, want_K=False, dtype=np.float64):
    """depth_bar (H, W); with want_K also K_bar (4, 4): the adjoint of the intrinsics through inverse_intrinsics
    (k00 = 1 / (fx + eps), k02 = -cx / (fx + eps), same for y; geometry/projutils.py:437-449), pinned against
    tests/golden/intrinsics_grad.npz.
    dtype: the precision every operation below is carried out in.  float64 is the oracle; float32 is the same formula
    at the kernels' precision, whose distance from the float64 result on a given input is the yardstick for what a
    float32 kernel may differ by on that input (tests/test_hip_backward_kernels.py)."""
    dt = np.dtype(dtype).type
    depth = np.asarray(depth, dt)
    H, W = depth.shape
    fx, fy = dt(float(K[0, 0]) + 1e-6), dt(float(K[1, 1]) + 1e-6)
    cx, cy = dt(float(K[0, 2])), dt(float(K[1, 2]))
    # inverse_intrinsics (geometry/projutils.py:444-449) in float32 like the reference
    k00, k11 = dt(np.float32(1.0) / np.float32(fx)), dt(np.float32(1.0) / np.float32(fy))
    k02, k12 = dt(-np.float32(cx) / np.float32(fx)), dt(-np.float32(cy) / np.float32(fy))
    w, h = np.meshgrid(np.arange(W, dtype=dt), np.arange(H, dtype=dt))
    ray = np.stack([k00 * w + k02, k11 * h + k12, np.ones_like(w)], -1)
    valid = (depth > 0).astype(dt)
    V = ray * (depth * valid)[..., None]
    Vb = np.array(v_bar, dt, copy=True)
    # alpha
    s = (V * V).sum(-1)
    two = dt(np.float32(2.0 * float(sigma) ** 2))
    e = np.exp(-s / two)
    inside = (e >= dt(np.float32(1e-7))) & (e <= dt(np.float32(1.01)))
    Vb += (np.asarray(a_bar, dt) * np.where(inside, e, dt(0)) * (dt(-2.0) / two))[..., None] * V
    # normals
    w0 = np.minimum(np.arange(W), W - 2)
    h0 = np.minimum(np.arange(H), H - 2)
    dh = V[:, w0 + 1] - V[:, w0]
    dv = V[h0 + 1] - V[h0]
    n = np.cross(dh, dv)
    nrm = np.sqrt((n * n).sum(-1))
    den = np.where(nrm == 0, dt(1), nrm)
    Nb = np.asarray(n_bar, dt) * valid[..., None]
    u = n / den[..., None]
    nb = (Nb - np.where(nrm == 0, dt(0), (Nb * u).sum(-1))[..., None] * u) / den[..., None]
    dh_b = np.cross(dv, nb)      # d(dh x dv): dh_bar = dv x n_bar, dv_bar = n_bar x dh
    dv_b = np.cross(nb, dh)
    np.add.at(Vb, (slice(None), w0 + 1), dh_b)
    np.add.at(Vb, (slice(None), w0), -dh_b)
    np.add.at(Vb, (h0 + 1,), dv_b)
    np.add.at(Vb, (h0,), -dv_b)
    depth_bar = (Vb * ray).sum(-1) * valid
    if not want_K:
        return depth_bar
    dm = depth * valid
    kb00, kb02 = (Vb[..., 0] * w * dm).sum(), (Vb[..., 0] * dm).sum()
    kb11, kb12 = (Vb[..., 1] * h * dm).sum(), (Vb[..., 1] * dm).sum()
    K_bar = np.zeros((4, 4), dt)
    K_bar[0, 0], K_bar[0, 2] = (-kb00 + kb02 * cx) / (fx * fx), -kb02 / fx
    K_bar[1, 1], K_bar[1, 2] = (-kb11 + kb12 * cy) / (fy * fy), -kb12 / fy
    return depth_bar, K_bar


def frame_maps_forward(depth, K, sigma):
    """float64 forward of the three maps (the formulas of the module docstring), for finite differences of the adjoint
    above.  K enters through the float64 inverse intrinsics here (no float32 rounding: a difference quotient needs a
    smooth function of K)."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    fx, fy, cx, cy = float(K[0, 0]) + 1e-6, float(K[1, 1]) + 1e-6, float(K[0, 2]), float(K[1, 2])
    w, h = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([w / fx - cx / fx, h / fy - cy / fy, np.ones_like(w)], -1)
    valid = (depth > 0).astype(np.float64)
    V = ray * (depth * valid)[..., None]
    w0 = np.minimum(np.arange(W), W - 2)
    h0 = np.minimum(np.arange(H), H - 2)
    n = np.cross(V[:, w0 + 1] - V[:, w0], V[h0 + 1] - V[h0])
    nrm = np.linalg.norm(n, axis=-1)
    N = n / np.where(nrm == 0, 1.0, nrm)[..., None] * valid[..., None]
    a = np.clip(np.exp(-(V * V).sum(-1) / (2.0 * float(sigma) ** 2)), 1e-7, 1.01)
    return V, N, a


# ---------------------------------------------------------------------------------------------- global maps
# structures/rgbdimages.py:681-762: gv = (R v + t) * valid, gn = R n with pose = [R t; 0 1]
def global_maps_forward(vertex, normal, depth, pose):
    pose = np.asarray(pose, np.float64)
    R, t = pose[:3, :3], pose[:3, 3]
    valid = (np.asarray(depth) > 0).astype(np.float64)[..., None]
    return (np.asarray(vertex, np.float64) @ R.T + t) * valid, np.asarray(normal, np.float64) @ R.T


def global_maps_backward(vertex, normal, depth, pose, gv_bar, gn_bar, dtype=np.float64):
    """(v_bar, n_bar, pose_bar): v_bar = R^T (gv_bar * valid), n_bar = R^T gn_bar,
    R_bar = sum_p valid gv_bar (x) v + sum_p gn_bar (x) n, t_bar = sum_p valid gv_bar, bottom row of pose_bar = 0.
    gv_bar / gn_bar may be None (that output carries no gradient): the matching result is None and its sum is left out."""
    dt = np.dtype(dtype).type
    pose = np.asarray(pose, dt)
    R = pose[:3, :3]
    valid = (np.asarray(depth) > 0).astype(dt)[..., None]
    pose_bar = np.zeros((4, 4), dt)
    v_bar = n_bar = None
    if gv_bar is not None:
        g = np.asarray(gv_bar, dt) * valid
        v_bar = g @ R
        pose_bar[:3, :3] += np.einsum("hwa,hwc->ac", g, np.asarray(vertex, dt))
        pose_bar[:3, 3] += g.sum((0, 1))
    if gn_bar is not None:
        g = np.asarray(gn_bar, dt)
        n_bar = g @ R
        pose_bar[:3, :3] += np.einsum("hwa,hwc->ac", g, np.asarray(normal, dt))
    return v_bar, n_bar, pose_bar


# ---------------------------------------------------------------------------------------------- lattice down-sampler
# odometry/icputils.py downsample_rgbdimages: the pixels (h, w) with h % ds == 0, w % ds == 0 and depth > 0, in raster order
def downsample_pixels(depth, ds):
    depth = np.asarray(depth)
    H, W = depth.shape
    hh, ww = np.meshgrid(np.arange(0, H, ds), np.arange(0, W, ds), indexing="ij")
    pix = (hh * W + ww).reshape(-1)
    return pix[depth.reshape(-1)[pix] > 0]


def downsample_forward(gvertex, depth, ds):
    g = np.asarray(gvertex)
    return g.reshape(-1, g.shape[-1])[downsample_pixels(depth, ds)]


def downsample_backward(pts_bar, depth, ds):
    """A scatter of copies: gvertex_bar[pixel of row k] = pts_bar[k], zero elsewhere (same dtype as pts_bar)."""
    pts_bar = np.asarray(pts_bar)
    H, W = np.asarray(depth).shape
    out = np.zeros((H * W, pts_bar.shape[-1]), pts_bar.dtype)
    out[downsample_pixels(depth, ds)] = pts_bar
    return out.reshape(H, W, -1)


# ---------------------------------------------------------------------------------------------- alpha of a point list
def alpha_backward(points, sigma, eps, a_bar, dtype=np.float64):
    """slam/fusionutils.py:69-72, a = clamp(exp(-|p|^2 / (2 sigma^2)), eps, 1.01): (points_bar (n, 3), sigma_bar)."""
    dt = np.dtype(dtype).type
    p = np.asarray(points, dt)
    S = (p * p).sum(-1)
    two = dt(np.float32(2.0 * float(sigma) ** 2))
    e = np.exp(-S / two)
    g = np.where((e >= dt(np.float32(eps))) & (e <= dt(np.float32(1.01))), np.asarray(a_bar, dt) * e, dt(0))
    return (g * (dt(-2.0) / two))[:, None] * p, (g * S).sum() / dt(float(sigma) ** 3)
