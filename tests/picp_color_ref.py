"""Restatement of the projective ICP's colour term (gradslam_amd/csrc/gs_picp_color.hip) in NumPy, on top of
tests/picp_ref.py (the geometric slot, the reduction, the solve) and tests/render_ref.py (the camera of the model view).
TEST INFRASTRUCTURE ONLY.

Everything added here is float32 with one rounding per operation and NO FMA (NumPy's float32 array arithmetic is exactly
that); the divisions are IEEE float32 divisions.

    luma(R, G, B) = (0.299f R + 0.587f G) + 0.114f B
    model intensity (H, W, 4) = (I, gx, gy, ok):  I = luma(rendered colour),
        ok = 1 iff the pixel and its 4 neighbours are inside the image and have index >= 0,
        gx = 0.5f (I[h, w+1] - I[h, w-1]), gy = 0.5f (I[h+1, w] - I[h-1, w]) where ok, else 0
    colour row of a used slot (code 0) whose model pixel (h2, w2) has ok = 1, s = T v, q = the camera-frame point of
    gs_project_point_hw_q (transform_points(s, Tinv)), (u, v) = the projector's continuous pixel
        r_j = ((K[j,0] q0 + K[j,1] q1) + K[j,2] q2) + K[j,3] * 1,  z = r_2 (1 if 0),  u = r_0 / z,  v = r_1 / z
        r   = Il - ((I + gx (u - w2)) + gy (v - h2)),   Il = luma(live colour at the slot's pixel)
        ax = gx K[0,0], ay = gy K[1,1];  Jq = (ax / q2, ay / q2, (-(ax q0 + ay q1)) / (q2 q2))
        Js_j = (R_m[j,0] Jq0 + R_m[j,1] Jq1) + R_m[j,2] Jq2
        c   = (Js2 s1 - Js1 s2, Js0 s2 - Js2 s0, Js1 s0 - Js0 s1)
        a_c = w (Js, c),  b_c = w r
    terms: (double)x_g (double)y_g + (double)x_c (double)y_c, each product exact, the sum rounded once."""
import collections
import math

import numpy as np

from oracle import oracle as o
from tests import picp_ref as pr
from tests import render_ref as rr

F = np.float32
ColorRows = collections.namedtuple("ColorRows", ["code", "row", "a", "b", "ac", "bc", "colored", "sums", "count",
                                                 "color_count"])
LUMA = (F(0.299), F(0.587), F(0.114))


def luma(rgb):
    rgb = np.asarray(rgb, F)
    t = LUMA[0] * rgb[..., 0] + LUMA[1] * rgb[..., 1]
    out = t + LUMA[2] * rgb[..., 2]
    assert out.dtype == F
    return out


def model_intensity(color, index):
    """(H, W, 4) float32 = (I, gx, gy, ok) of one view: color (H, W, 3), index (H, W)"""
    I = luma(color)
    H, W = I.shape
    hit = np.zeros((H + 2, W + 2), bool)
    hit[1:-1, 1:-1] = np.asarray(index) >= 0
    ok = hit[1:-1, 1:-1] & hit[1:-1, :-2] & hit[1:-1, 2:] & hit[:-2, 1:-1] & hit[2:, 1:-1]
    Ip = np.zeros((H + 2, W + 2), F)
    Ip[1:-1, 1:-1] = I
    gx = F(0.5) * (Ip[1:-1, 2:] - Ip[1:-1, :-2])
    gy = F(0.5) * (Ip[2:, 1:-1] - Ip[:-2, 1:-1])
    out = np.zeros((H, W, 4), F)
    out[..., 0] = I
    out[..., 1] = np.where(ok, gx, F(0))
    out[..., 2] = np.where(ok, gy, F(0))
    out[..., 3] = ok
    return out


def projector(s, model_pose, K, H, W):
    """q (n, 3), u, v (n,) float32 and the clamped rounded pixel (h2, w2) of gs_project_point_hw_q, for every s (the
    in-frame test is the caller's: used slots passed it)"""
    Tinv, _ = rr.camera_inverse(model_pose)
    q = o.transform_points(np.ascontiguousarray(s, F), Tinv)
    K = np.asarray(K, F)
    r = []
    for j in range(3):
        acc = K[j, 0] * q[:, 0]
        acc = acc + K[j, 1] * q[:, 1]
        acc = acc + K[j, 2] * q[:, 2]
        acc = acc + K[j, 3] * F(1)
        r.append(acc)
    with np.errstate(all="ignore"):
        zz = np.where(r[2] != 0, r[2], F(1))
        u, v = r[0] / zz, r[1] / zz
        w2 = np.clip(np.rint(np.nan_to_num(u, nan=0.0, posinf=0.0, neginf=0.0)), 0, W - 1).astype(np.int64)
        h2 = np.clip(np.rint(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)), 0, H - 1).astype(np.int64)
    assert u.dtype == F and v.dtype == F
    return q, u, v, h2, w2


def color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight):
    """(ac (n, 6), bc (n,), colored bool (n,)) of the slots whose geometric codes are `code`"""
    H, W = model.shape[:2]
    v = np.ascontiguousarray(np.asarray(vertex, F)[::stride, ::stride]).reshape(-1, 3)
    col = np.ascontiguousarray(np.asarray(color, F)[::stride, ::stride]).reshape(-1, 3)
    ns = v.shape[0]
    ac, bc, colored = np.zeros((ns, 6), F), np.zeros(ns, F), np.zeros(ns, bool)
    used = np.nonzero(code == 0)[0]
    if not used.size:
        return ac, bc, colored
    T = np.asarray(T, F).reshape(4, 4)
    K = np.asarray(K, F)
    s = o.transform_points(np.ascontiguousarray(v[used]), T)
    q, u, vv, h2, w2 = projector(s, model_pose, K, H, W)
    # the pixel is the one the association read
    assert np.array_equal(h2 * W + w2, o.project_map(s, model_pose, K, H, W).astype(np.int64))
    M = np.asarray(model, F)[h2, w2]
    sel = M[:, 3] == 1
    colored[used[sel]] = True
    s, q, u, vv, h2, w2, M = s[sel], q[sel], u[sel], vv[sel], h2[sel], w2[sel], M[sel]
    I, gx, gy = M[:, 0], M[:, 1], M[:, 2]
    Il = luma(col[used[sel]])
    lin = I + gx * (u - w2.astype(F))
    r = Il - (lin + gy * (vv - h2.astype(F)))
    ax, ay = gx * K[0, 0], gy * K[1, 1]
    j0, j1 = ax / q[:, 2], ay / q[:, 2]
    j2 = (-(ax * q[:, 0] + ay * q[:, 1])) / (q[:, 2] * q[:, 2])
    R = np.asarray(model_pose, F).reshape(4, 4)[:3, :3]
    J = [(R[j, 0] * j0 + R[j, 1] * j1) + R[j, 2] * j2 for j in range(3)]
    w = F(weight)
    out = [w * J[0], w * J[1], w * J[2],
           w * (J[2] * s[:, 1] - J[1] * s[:, 2]),
           w * (J[0] * s[:, 2] - J[2] * s[:, 0]),
           w * (J[1] * s[:, 0] - J[0] * s[:, 1])]
    for c in range(6):
        assert out[c].dtype == F
        ac[used[sel], c] = out[c]
    bc[used[sel]] = w * r
    assert r.dtype == F
    return ac, bc, colored


def joint_terms(code, a, b, ac, bc):
    """(n, 28) float64: the geometric product plus the colour product, each exact, the sum rounded once"""
    g, c = pr.terms(code, a, b), pr.terms(code, ac, bc)
    return g + c


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight, stride=1,
         dist_thresh=0.1, angle_thresh=30.0):
    """one joint linearisation at T"""
    dist_th, dot_th = pr.thresholds(dist_thresh, angle_thresh)
    code, row, a, b = pr.slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride,
                                   dist_th, dot_th)
    ac, bc, colored = color_slot_rows(code, vertex, color, K, model, model_pose, T, stride, weight)
    sums = pr.reduce_terms(joint_terms(code, a, b, ac, bc))
    return ColorRows(code, row, a, b, ac, bc, colored, sums, int((code == 0).sum()), int(colored.sum()))


def solve(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T0, weight, stride=1,
          numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30.0):
    """(pose (4, 4), trace (numiters, 9) = [count, (float) joint S[27], xi(6), colour rows])"""
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 9), F)
    for it in range(numiters):
        r = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, color, model, T, weight, stride,
                 dist_thresh, angle_thresh)
        xi = np.zeros(6, F)
        if r.count > 0:        # no geometric inlier: xi = 0 and T keeps its bits
            xi = pr.solve_spd6(r.sums, damp)
            T = pr.mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:8], trace[it, 8] = F(r.count), F(r.sums[27]), xi, F(r.color_count)
    return T, trace


# ------------------------------------------------------------------------------------------ the textured fixture
SCENES = {"plane": lambda x, y: 2.0 + 0.0 * x, "tilted": lambda x, y: 2.0 + 0.2 * x}


def texture(x, y):
    """A smooth world-anchored texture, three different channels in [0, 1] that use most of that range.  Wavelengths of
    0.9 m to 2.5 m against a 30 mm pixel (60 x 80 at 2 m): at least 30 pixels per wave, so the first-order model of the
    colour row holds within a pixel, and a luma gradient of a few percent of the range per pixel, so that the colour rows
    outweigh what the geometric rows pull along a plane (the frame normals next to the 5 % holes are not the plane's)."""
    r = 0.5 + 0.45 * np.sin(6.0 * x + 0.3) * np.cos(5.0 * y)
    g = 0.5 + 0.3 * np.cos(7.0 * x - 3.0 * y + 1.0) + 0.15 * np.sin(5.5 * y)
    b = 0.5 + 0.45 * np.sin(2.5 * x + 4.5 * y) * np.cos(3.0 * x - 0.7)
    return np.stack([r, g, b], -1)


_SEQ = {}


def textured_sequence(L=6, H=60, W=80, scene="plane", seed=0):
    """make_sequence's camera path, intrinsics and 5 % holes on `scene` ("wave": make_sequence's own depths; "plane",
    "tilted": ray-cast here by the same fixed-point iteration), with colours = texture(world x, world y) of the surface
    point a pixel sees, in [0, 1] (0 in a hole).  Cached and read-only."""
    key = (L, H, W, scene, seed)
    if key in _SEQ:
        return _SEQ[key]
    from gradslam_amd.datasets.synthetic import gt_pose, make_sequence, tum_intrinsics
    K = tum_intrinsics(H, W)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rx, ry = (uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1]
    if scene == "wave":
        s = make_sequence(L, H, W, seed=seed, scene="wave")
        depths, poses = s["depths"], s["poses"]
    else:
        rng = np.random.default_rng(seed)
        depths, poses = np.empty((L, H, W, 1), F), np.empty((L, 4, 4), F)
        for f in range(L):
            T = gt_pose(f).astype(np.float64)
            poses[f] = T.astype(F)
            d = np.full((H, W), 2.0)
            for _ in range(30):
                pw = np.stack([rx * d, ry * d, d], -1) @ T[:3, :3].T + T[:3, 3]
                d = d + (SCENES[scene](pw[..., 0], pw[..., 1]) - pw[..., 2]) / T[2, 2]
            depths[f, ..., 0] = np.where(rng.random((H, W)) < 0.05, 0.0, d).astype(F)
    colors = np.zeros((L, H, W, 3), F)
    for f in range(L):
        d = depths[f, ..., 0].astype(np.float64)
        T = poses[f].astype(np.float64)
        pw = np.stack([rx * d, ry * d, d], -1) @ T[:3, :3].T + T[:3, 3]
        colors[f] = np.where((d > 0)[..., None], texture(pw[..., 0], pw[..., 1]), 0.0).astype(F)
    seq = {"colors": colors, "depths": depths, "intrinsics": K[None], "poses": poses}
    for val in seq.values():
        val.setflags(write=False)
    _SEQ[key] = seq
    return seq


_FIXTURES = {}
ARGS = pr.ARGS + ("color", "model")


def textured_fixture(H=60, W=80, frame=5, scene="plane"):
    """frame `frame` of textured_sequence against a map of frame 0's valid pixels (with their colours), the index and
    colour images of tests/render_ref.py at pose 0 and their model intensity.  Cached and read-only."""
    key = (H, W, frame, scene)
    if key not in _FIXTURES:
        s = textured_sequence(6, H, W, scene)
        K, pose0 = s["intrinsics"][0], s["poses"][0]
        d0 = s["depths"][0, ..., 0]
        P, N, _, Fc = pr.frame_map(d0, K, pose0)
        _, _, _, valid = o.frame_maps(d0, K)
        Cc = np.ascontiguousarray(s["colors"][0][valid])
        view = rr.render(P, N, Cc, Fc, pose0, K, H, W)
        depth = np.ascontiguousarray(s["depths"][frame, ..., 0])
        v, n, _, _ = o.frame_maps(depth, K)
        fx = dict(vertex=v, normal=n, depth=depth, K=K, index=view.index, model_pose=pose0, points=P, normals=N,
                  count=P.shape[0], color=np.ascontiguousarray(s["colors"][frame]),
                  model=model_intensity(view.color, view.index), view_color=view.color, map_colors=Cc, T0=pose0,
                  gt=s["poses"][frame], seq=s)
        for val in fx.values():
            if isinstance(val, np.ndarray):
                val.setflags(write=False)
        _FIXTURES[key] = fx
    return _FIXTURES[key]


def args_of(fx):
    return [fx[k] for k in ARGS]


def run_sequence(seq, weight, stride=1, numiters=10, dist_th=0.05, angle_th=20, sigma=0.6, **kw):
    """tests/picp_ref.run_sequence with the joint solve (weight > 0) or the plain one (weight == 0): the PointFusion frame
    loop on the oracle's map.  Returns the poses (L, 4, 4)."""
    from oracle import slam as oslam
    depths = seq["depths"][..., 0]
    K = seq["intrinsics"][0]
    L, H, W = depths.shape
    dot_th = math.cos((angle_th * math.pi) / 180)
    m = oslam.MapState()
    poses = np.zeros((L, 4, 4), F)
    for f in range(L):
        depth, rgb = np.ascontiguousarray(depths[f]), seq["colors"][f]
        v, n, a, _ = o.frame_maps(depth, K, sigma)
        if f == 0:
            pose = np.array(seq["poses"][0], F)
        else:
            view = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[f - 1], K, H, W)
            geo = (v, n, depth, K, view.index, poses[f - 1], m.points, m.normals, len(m))
            if weight > 0:
                pose, _ = solve(*geo, rgb, model_intensity(view.color, view.index), poses[f - 1], weight, stride=stride,
                                numiters=numiters, **kw)
            else:
                pose, _ = pr.solve(*geo, poses[f - 1], stride=stride, numiters=numiters, **kw)
        gv, gn = o.global_maps(v, n, depth, pose)
        if len(m):
            best, _ = o.associate(o.project_map(m.points, pose, K, H, W), m.points, m.normals, m.ccounts, gv, gn,
                                  dist_th, dot_th)
        else:
            best = np.full(H * W, -1, np.int32)
        m.points, m.normals, m.colors, m.ccounts = o.fuse_append(m.points, m.normals, m.colors, m.ccounts, best, gv, gn,
                                                                 rgb, a, depth, True)
        poses[f] = pose
    return poses
