"""Surfel radii restated in NumPy: the radius of a depth sample (gradslam_amd/csrc/gs_radii.hip), the splat size it
turns into in a view (gs_render.hip, the radii entries) and the oracle frame loop with a SurfelRadii layer between the
frames.  TEST INFRASTRUCTURE ONLY.

Every float32 operation is one NumPy float32 operation (one rounding each, no FMA):

    fbar  = 0.5f * (K[0,0] + K[1,1])
    r0    = (0.70710678f * z) / fbar
    c     = fabsf(n_z)
    rho   = fminf(r0 / c, 2.0f * r0)          (c == 0: 2.0f * r0)
    valid = z > 0 and n finite and not all zero;  rho = +0.0f where not valid

    x = (rho * fbar) / q2;   r = (rho > 0 and 0 < x < inf) ? min(max_radius, (int)floorf(x)) : 0

The layer rule is the feature-layer rule (tests/feature_fuse_ref.fuse) on the radius image with the colours' weights."""
import math

import numpy as np

from oracle import oracle as o
from tests import feature_fuse_ref as ffr

f32 = np.float32


def fbar_of(K):
    K = np.asarray(K, f32).reshape(4, 4)
    return f32(0.5) * (K[0, 0] + K[1, 1])


def surfel_radius(depth, normal, K):
    """depth (H, W), normal (H, W, 3) local normals, K (4, 4) -> (radius (H, W) float32, valid (H, W) bool)"""
    z = np.asarray(depth, f32)
    n = np.asarray(normal, f32).reshape(z.shape + (3,))
    with np.errstate(all="ignore"):
        r0 = (f32(0.70710678) * z) / fbar_of(K)
        c = np.abs(n[..., 2])
        cap = f32(2.0) * r0
        rho = np.where(c == 0, cap, np.fmin(r0 / np.where(c == 0, f32(1.0), c), cap))
        valid = (z > 0) & np.isfinite(n).all(-1) & ~(n == 0).all(-1)
    assert rho.dtype == f32
    return np.where(valid, rho, f32(0.0)).astype(f32), valid


def splat_radius(rho, K, q2, max_radius):
    """the half-width in pixels of rows of radius rho (n,) at camera-frame depth q2 (n,) > 0: int64 (n,)"""
    rho, q2 = np.asarray(rho, f32), np.asarray(q2, f32)
    with np.errstate(all="ignore"):
        x = (rho * fbar_of(K)) / q2
        assert x.dtype == f32
        ok = (rho > 0) & (x > 0) & (x < np.inf)
        r = np.where(ok, np.minimum(np.floor(np.where(ok, x, 0)), max_radius), 0)
    return r.astype(np.int64)


class Layer:
    """a SurfelRadii layer of one sequence next to an oracle map: radius (n,) and weight (n,)"""

    def __init__(self):
        self.radius, self.weight = np.zeros(0, f32), np.zeros(0, f32)


def run_sequence(colors, depths, K, poses, *, dist_th=0.05, angle_th=20, sigma=0.6, renorm_all=True, carve=None,
                 voxel_size=None, prune=None, per_frame=None):
    """oracle.slam.run_sequence(slam="pointfusion", odom="gt") with the layer rule after every map update and, like
    PointFusion.step, the schedules after it: carve = dict(margin, window) every step against the frame just fused,
    voxel_size every step, prune = dict(min_confidence, every) with min_age 0.  Every removal compacts the layer by the
    mask that compacts the map.  Returns (oracle map, Layer)."""
    from oracle import slam as oslam
    from tests import carve_ref, prune_ref, voxel_ref
    depths = np.asarray(depths, f32).reshape(depths.shape[0], depths.shape[1], depths.shape[2])
    L, H, W = depths.shape
    K = np.asarray(K, f32).reshape(4, 4)
    dot_th = math.cos((angle_th * math.pi) / 180)
    m, lay = oslam.MapState(), Layer()

    def compact(keep):
        keep = np.asarray(keep[:len(m)]) != 0
        m.points, m.normals, m.colors, m.ccounts = (a[keep] for a in (m.points, m.normals, m.colors, m.ccounts))
        lay.radius, lay.weight = lay.radius[keep], lay.weight[keep]

    for s in range(L):
        depth, rgb, pose = depths[s], np.asarray(colors[s], f32), np.asarray(poses[s], f32)
        v, n, a, _ = o.frame_maps(depth, K, sigma)
        gv, gn = o.global_maps(v, n, depth, pose)
        n_old = len(m)
        if n_old:
            pix = o.project_map(m.points, pose, K, H, W)
            best, _ = o.associate(pix, m.points, m.normals, m.ccounts, gv, gn, dist_th, dot_th)
        else:
            best = np.full(H * W, -1, np.int32)
        m.points, m.normals, m.colors, m.ccounts = o.fuse_append(
            m.points, m.normals, m.colors, m.ccounts, best, gv, gn, rgb, a, depth, renorm_all)
        feat, valid = surfel_radius(depth, n, K)
        emb = np.zeros((n_old + H * W, 1), f32)
        wgt = np.zeros(n_old + H * W, f32)
        emb[:n_old, 0], wgt[:n_old] = lay.radius, lay.weight
        emb, wgt, _, n_new = ffr.fuse(emb, wgt, n_old, best, depth, a, feat.reshape(H, W, 1), valid.reshape(-1))
        assert n_new == len(m)
        lay.radius, lay.weight = emb[:n_new, 0].copy(), wgt[:n_new].copy()
        if carve is not None:
            compact(carve_ref.free_space(m.points, len(m), [depth], [pose], K, carve["margin"], carve["window"], 1)[1])
        if voxel_size is not None:
            compact(voxel_ref.voxel_keep(m.points, m.ccounts, len(m), voxel_size)[0])
        if prune is not None and (s + 1) % prune["every"] == 0:
            compact(prune_ref.survivors(len(m), m.ccounts, prune["min_confidence"]))
        if per_frame is not None:
            per_frame(s, m, lay)
    return m, lay
