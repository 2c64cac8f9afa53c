"""NumPy restatement of the free-space carve (gradslam_amd/csrc/gs_carve.hip -> gs_free_space_dc_f32 ->
ops.free_space_batch -> Pointclouds.carve_), built only from pieces that are already pinned to the reference:
`oracle.project_map` for the pixel a map row lands on, and `tests.render_ref.camera_inverse` + `oracle.transform_points`
for its camera-frame depth z (the composition `render_ref.row_keys` uses).  TEST INFRASTRUCTURE ONLY.

Row r < n violates view l (pose T_l, depth image D_l) iff

    pix[r] >= 0                                   (it projects into the frame, in front of the camera)
    D_l[h, w] > 0                                 (false for 0, negative depths and NaN)
    for every (hh, ww) of the (2 window + 1)^2 square around (h, w), clipped to the image, with D_l[hh, ww] > 0:
        (D_l[hh, ww] - z) > margin                (float32: one subtraction, one compare; equality does not violate)

violations[r] = number of views r violates, keep[r] = violations[r] < min_views; rows in [n, n_bound) hold 0 in both."""
import numpy as np

from oracle import oracle as o
from tests import render_ref as rr


def project(points, pose, K, H, W):
    """(pix int64 (n,): h * W + w or -1, z float32 (n,)): the pixel and the camera-frame depth of every row"""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if points.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    pix = o.project_map(points, pose, K, H, W).astype(np.int64)
    Tinv, _ = rr.camera_inverse(pose)
    z = np.ascontiguousarray(o.transform_points(points, Tinv)[:, 2])
    assert z.dtype == np.float32
    return pix, z


def violates(points, depth, pose, K, margin=0.05, window=1):
    """(n,) bool: which rows violate the one view."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    depth = np.ascontiguousarray(depth, np.float32)
    H, W = depth.shape[:2]
    depth = depth.reshape(H, W)
    n = points.shape[0]
    if n == 0:
        return np.zeros(0, bool)
    pix, z = project(points, pose, K, H, W)
    margin = np.float32(margin)
    inside = pix >= 0
    h, w = np.where(inside, pix // W, 0), np.where(inside, pix % W, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        centre = depth[h, w]
        out = inside & (centre > 0)
        for dh in range(-window, window + 1):
            for dw in range(-window, window + 1):
                hh, ww = h + dh, w + dw
                ok = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
                d = depth[np.clip(hh, 0, H - 1), np.clip(ww, 0, W - 1)]
                diff = d - z
                assert diff.dtype == np.float32
                measured = ok & (d > 0)
                out &= ~measured | (diff > margin)
    return out


def free_space(points, n, depths, poses, K, margin=0.05, window=1, min_views=1):
    """One sequence: points (n_bound, 3) of which the first n are the map, depths (L, H, W[, 1]), poses (L, 4, 4).
    Returns (violations int32 (n_bound,), keep uint8 (n_bound,))."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n_bound, n = points.shape[0], int(n)
    viol = np.zeros(n_bound, np.int32)
    for l in range(len(depths)):
        viol[:n] += violates(points[:n], depths[l], poses[l], K, margin, window)
    keep = np.zeros(n_bound, np.uint8)
    keep[:n] = viol[:n] < min_views
    return viol, keep


def ghost_rows(points, depth_clean, pose, K, ahead=0.2):
    """rows that lie more than `ahead` metres in front of the clean depth of their pixel in the view"""
    depth_clean = np.asarray(depth_clean, np.float32)
    H, W = depth_clean.shape[:2]
    pix = o.project_map(np.ascontiguousarray(points, np.float32), pose, K, H, W).astype(np.int64)
    z = o.transform_points(np.ascontiguousarray(points, np.float32), rr.camera_inverse(pose)[0])[:, 2]
    d = depth_clean.reshape(-1)[np.where(pix >= 0, pix, 0)]
    return int(((pix >= 0) & (d > 0) & (d.astype(np.float64) - z.astype(np.float64) > ahead)).sum())


# the demonstration: a block of pixels that stands 0.4 m nearer to the camera in the first frames and is gone after them
SEQ_L, SEQ_H, SEQ_W = 12, 60, 80
BLOCK = (slice(20, 40), slice(30, 50))
BLOCK_FRAMES, BLOCK_SHIFT = 6, np.float32(0.4)


def block_sequence(scene="wave", moved=True):
    """make_sequence(12, 60, 80) of `scene`; with `moved`, the measured pixels of a 20 x 20 block are 0.4 m nearer in
    frames 0..5.  Also returns the undisturbed depths under "clean"."""
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(SEQ_L, SEQ_H, SEQ_W, seed=0, scene=scene)
    s["clean"] = s["depths"].copy()
    if moved:
        blk = s["depths"][(slice(0, BLOCK_FRAMES),) + BLOCK]
        s["depths"][(slice(0, BLOCK_FRAMES),) + BLOCK] = np.where(blk > 0, blk - BLOCK_SHIFT, blk).astype(np.float32)
    return s


def carve_map(m, depth, pose, K, margin=0.05, window=1):
    """The carve of one step on an oracle map (oracle.slam's surfel store: points / normals / colors / ccounts), in
    place: L = 1, min_views = 1.  Returns the number of rows removed."""
    n = len(m)
    _, keep = free_space(m.points, n, [depth], [pose], K, margin, window, 1)
    s = keep != 0
    m.points, m.normals, m.colors, m.ccounts = (np.ascontiguousarray(a[:n][s]) for a in
                                                (m.points, m.normals, m.colors, m.ccounts))
    return n - int(s.sum())
