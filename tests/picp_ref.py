"""Restatement of the projective-association ICP (gradslam_amd/csrc/gs_picp.hip) in NumPy.  TEST INFRASTRUCTURE ONLY.

The per-slot stage is float32, one rounding per operation, and takes every chain that contains an FMA from the oracle,
where it is pinned already:

    s    = transform_points(v, T)                 s_j = fma(T[j,2], v2, fma(T[j,1], v1, T[j,0] * v0)) + T[j,3]
    g    = transform_points(n, [R_T | 0])         the same chain; the + 0 only turns a -0 into +0, which no comparison sees
    pix  = project_map(s, model_pose, K, H, W)    gs_camera + gs_project_point_hw
    gate = similar_rows(...)                      dist = norm3(s - p) < dist_th, then dot_plain(g, m) > dot_th
    row  = the plain float32 products and differences of gn_row_pn

Codes: 0 used, 1 no depth, 2 outside the model view, 3 no (or a stale) winner, 4 too far, 5 normals disagree.
The 28 terms are exact float64 products of float32 factors.  Reduction order (part of the contract): chunks of 256
consecutive slots (the tail padded with +0.0), inside a chunk a pairwise adjacent tree of 8 levels, the chunk partials
added in ascending chunk order starting from the first partial.  The solve is the un-pivoted Gauss-Jordan elimination of
gs_solve_spd<6> in float64 on the float32-rounded system, the step se3_exp (oracle) and the 4x4 product of the ICP loop."""
import collections
import math

import numpy as np

from oracle import oracle as o

CHUNK = 256
NV = 28
Rows = collections.namedtuple("Rows", ["code", "row", "a", "b", "sums", "count"])
F = np.float32


def thresholds(dist_thresh=0.1, angle_thresh=30.0):
    """the float32 casts of the Python doubles, as the kernels receive them"""
    return F(dist_thresh), F(math.cos(angle_thresh * math.pi / 180))


def lattice_shape(H, W, stride):
    return (H + stride - 1) // stride, (W + stride - 1) // stride


def slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th, dot_th):
    """per-slot stage: (code int32 (n,), row int64 (n,), a float32 (n, 6), b float32 (n,)).  row = the index image's
    entry where one was read (codes 0, 3, 4, 5), else -1; a, b = 0 unless the slot is used."""
    depth = np.asarray(depth, F)
    H, W = depth.shape
    v = np.ascontiguousarray(np.asarray(vertex, F)[::stride, ::stride]).reshape(-1, 3)
    n = np.ascontiguousarray(np.asarray(normal, F)[::stride, ::stride]).reshape(-1, 3)
    d = np.ascontiguousarray(depth[::stride, ::stride]).reshape(-1)
    ns = d.shape[0]
    T = np.asarray(T, F).reshape(4, 4)
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    count = max(0, min(int(count), points.shape[0]))
    index = np.asarray(index, np.int64).reshape(-1)
    code = np.zeros(ns, np.int32)
    row = np.full(ns, -1, np.int64)
    a = np.zeros((ns, 6), F)
    b = np.zeros(ns, F)
    with np.errstate(invalid="ignore"):
        code[~(d > 0)] = 1
    s = o.transform_points(v, T)
    Trot = T.copy()
    Trot[:3, 3] = 0.0
    g = o.transform_points(n, Trot)
    pix = o.project_map(s, model_pose, K, H, W).astype(np.int64)
    code[(code == 0) & (pix < 0)] = 2
    live = code == 0
    row[live] = index[pix[live]]
    code[live & ((row < 0) | (row >= count))] = 3
    live = np.nonzero(code == 0)[0]
    if live.size:
        r = row[live]
        table = np.stack([np.zeros_like(live), r, np.zeros_like(live), live], 1).astype(np.int64)
        near = o.similar_rows(table, points, normals, s.reshape(1, ns, 3), g.reshape(1, ns, 3), dist_th, F(-np.inf))
        both = o.similar_rows(table, points, normals, s.reshape(1, ns, 3), g.reshape(1, ns, 3), dist_th, dot_th)
        code[live[~near]] = 4
        code[live[near & ~both]] = 5
    live = np.nonzero(code == 0)[0]
    if live.size:
        p, m, q = points[row[live]], normals[row[live]], s[live]
        sx, sy, sz = q[:, 0], q[:, 1], q[:, 2]
        dx, dy, dz = p[:, 0], p[:, 1], p[:, 2]
        nx, ny, nz = m[:, 0], m[:, 1], m[:, 2]
        a[live, 0], a[live, 1], a[live, 2] = nx, ny, nz
        a[live, 3] = nz * sy - ny * sz
        a[live, 4] = nx * sz - nz * sx
        a[live, 5] = ny * sx - nx * sy
        t = nx * (dx - sx) + ny * (dy - sy)
        b[live] = t + nz * (dz - sz)
        assert a.dtype == F and b.dtype == F and t.dtype == F
    return code, row, a, b


def terms(code, a, b):
    """(n, 28) exact float64 terms in the S layout: 21 upper-triangular a_i a_j, 6 a_i b, b b; +0.0 for rejected slots"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    cols = [a64[:, i] * a64[:, j] for i in range(6) for j in range(i, 6)]
    cols += [a64[:, i] * b64 for i in range(6)]
    cols.append(b64 * b64)
    t = np.stack(cols, 1)
    t[code != 0] = 0.0
    return t


def reduce_terms(t):
    """the contract's order: 256-slot chunks, pairwise adjacent tree, partials in ascending chunk order"""
    n = t.shape[0]
    nchunks = max(1, (n + CHUNK - 1) // CHUNK)
    x = np.zeros((nchunks * CHUNK, t.shape[1]), np.float64)
    x[:n] = t
    x = x.reshape(nchunks, CHUNK, t.shape[1])
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    part = x[:, 0]
    S = part[0].copy()
    for c in range(1, nchunks):
        S = S + part[c]
    return S


def rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride=1, dist_thresh=0.1,
         angle_thresh=30.0):
    """one linearisation at T: Rows(code, row, a, b, sums float64 (28,), count)"""
    dist_th, dot_th = thresholds(dist_thresh, angle_thresh)
    code, row, a, b = slot_rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_th,
                                dot_th)
    return Rows(code, row, a, b, reduce_terms(terms(code, a, b)), int((code == 0).sum()))


def solve_spd6(S, damp):
    """gs_solve_spd<6> on (float)S: float32 system, damping added in float32, Gauss-Jordan in float64, rounded once"""
    damp = F(damp)
    A = np.zeros((6, 7), np.float64)
    q = 0
    sym = np.zeros((6, 6), F)
    for i in range(6):
        for k in range(i, 6):
            sym[i, k] = sym[k, i] = F(S[q])
            q += 1
    for i in range(6):
        for j in range(6):
            e = F(1.0) if i == j else F(0.0)
            A[i, j] = np.float64(F(sym[i, j] + F(e * damp)))
        A[i, 6] = np.float64(F(S[21 + i]))
    for c in range(6):
        inv = 1.0 / A[c, c]
        for j in range(c, 7):
            A[c, j] = A[c, j] * inv
        for r in range(6):
            if r == c:
                continue
            f = A[r, c]
            for j in range(c, 7):
                A[r, j] = A[r, j] - f * A[c, j]
    return A[:, 6].astype(F)


def mm4(A, B):
    """the 4x4 product of the ICP loop: plain float32, k ascending"""
    A, B = np.asarray(A, F), np.asarray(B, F)
    C = np.empty((4, 4), F)
    for i in range(4):
        for j in range(4):
            acc = F(A[i, 0] * B[0, j])
            for k in range(1, 4):
                acc = F(acc + F(A[i, k] * B[k, j]))
            C[i, j] = acc
    return C


def solve(vertex, normal, depth, K, index, model_pose, points, normals, count, T0, stride=1, numiters=10, damp=1e-8,
          dist_thresh=0.1, angle_thresh=30.0):
    """(pose float32 (4, 4), trace float32 (numiters, 8) = [count, (float)S[27], xi(6)] per iteration)"""
    T = np.array(T0, F).reshape(4, 4).copy()
    trace = np.zeros((numiters, 8), F)
    for it in range(numiters):
        r = rows(vertex, normal, depth, K, index, model_pose, points, normals, count, T, stride, dist_thresh,
                 angle_thresh)
        xi = np.zeros(6, F)
        if r.count > 0:        # no inlier: xi = 0 and T keeps its bits
            xi = solve_spd6(r.sums, damp)
            T = mm4(o.se3_exp(xi), T)
        trace[it, 0], trace[it, 1], trace[it, 2:] = F(r.count), F(r.sums[27]), xi
    return T, trace


# ------------------------------------------------------------------------------------------ fixtures of the tests
def frame_map(depth, K, pose):
    """a map made of one frame's valid pixels under `pose` (raster order): points, normals, colours 0, counts 1"""
    v, n, _, valid = o.frame_maps(depth, K)
    gv, gn = o.global_maps(v, n, depth, pose)
    P, N = np.ascontiguousarray(gv[valid]), np.ascontiguousarray(gn[valid])
    return P, N, np.zeros_like(P), np.ones((P.shape[0], 1), F)


_FIXTURES = {}


def convergence_fixture(H=60, W=80, frame=5, scene="wave"):
    """frame `frame` of make_sequence(6, H, W, seed=0, scene) against a map of frame 0's valid pixels, the index image
    of tests/render_ref.py at pose 0.  Cached and read-only."""
    key = (H, W, frame, scene)
    if key not in _FIXTURES:
        from gradslam_amd.datasets.synthetic import make_sequence
        from tests import render_ref as rr
        s = make_sequence(6, H, W, seed=0, scene=scene)
        K = s["intrinsics"][0]
        pose0 = s["poses"][0]
        P, N, Cc, Fc = frame_map(s["depths"][0, ..., 0], K, pose0)
        index = rr.render(P, N, Cc, Fc, pose0, K, H, W).index
        depth = np.ascontiguousarray(s["depths"][frame, ..., 0])
        v, n, _, _ = o.frame_maps(depth, K)
        fx = dict(vertex=v, normal=n, depth=depth, K=K, index=index, model_pose=pose0, points=P, normals=N,
                  count=P.shape[0], T0=pose0, gt=s["poses"][frame], seq=s)
        for val in fx.values():
            if isinstance(val, np.ndarray):
                val.setflags(write=False)
        _FIXTURES[key] = fx
    return _FIXTURES[key]


ARGS = ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals", "count")


def args_of(fx):
    return [fx[k] for k in ARGS]


def run_sequence(seq, stride=1, numiters=10, dist_th=0.05, angle_th=20, sigma=0.6, **kw):
    """The PointFusion frame loop with the restatement as odometry: frame 0 at its given pose, every later frame
    localised against the model view at the previous pose (tests/render_ref.py) from that pose, then the oracle's
    fusion update.  Returns (oracle MapState, poses (L, 4, 4))."""
    from oracle import slam as oslam
    from tests import render_ref as rr
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
            index = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[f - 1], K, H, W).index
            pose, _ = solve(v, n, depth, K, index, poses[f - 1], m.points, m.normals, len(m), poses[f - 1],
                            stride=stride, numiters=numiters, **kw)
        gv, gn = o.global_maps(v, n, depth, pose)
        if len(m):
            best, _ = o.associate(o.project_map(m.points, pose, K, H, W), m.points, m.normals, m.ccounts, gv, gn,
                                  dist_th, dot_th)
        else:
            best = np.full(H * W, -1, np.int32)
        m.points, m.normals, m.colors, m.ccounts = o.fuse_append(m.points, m.normals, m.colors, m.ccounts, best, gv, gn,
                                                                 rgb, a, depth, True)
        poses[f] = pose
    return m, poses
