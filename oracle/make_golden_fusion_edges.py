"""Constructed edge scenes of the map update, recorded from the REAL reference (gradslam v0.1.0 through
oracle/refimport.py): find_active_map_points, find_similar_map_points, find_best_unique_correspondences and fuse_with_map
(slam/fusionutils.py:198-722) on CPU torch.

    python -m oracle.make_golden_fusion_edges        ->  tests/golden/fusion_edges.npz

Before writing, the C oracle (oracle/oracle.py) is run on the same inputs and must reproduce the reference: tables, masks
and counts bit-exact, fused values bit-exact when fed the reference's alpha and global maps
(oracle/fusion_edges.py:assert_oracle_is_reference).  Build-container only; oracle/fusion_edges.py reads the file.

Two camera kinds.  EXACT: identity or axis-permutation pose with a dyadic translation, power-of-two focal lengths, dyadic
principal point, map points on a dyadic grid -- every intermediate of the projection is exact in float32 and the pixel of
every row is ALSO written down by hand (expect_pix, from exact rational arithmetic, never from the code under test).
GENERAL: a rotated pose, a non-square K with a negative fy.

What the reference cannot record (kept as notes, not as quirks of the oracle):
  * a frame with H == 1 or W == 1: RGBDImages._compute_normal_map indexes column / row -2 (rgbdimages.py:730-731).  The
    1x1 scene is therefore recorded with meta ref = 0: its maps and outputs are the C oracle's, and every expected value
    of it is one literal (a single pixel).  The smallest frame the reference runs, 2x2, is recorded next to it.
  * alpha == 0: get_alpha clamps to 1e-7.  The GPU test covers that merge at table level against the oracle alone."""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle import fusion_edges as fe  # noqa: E402
from oracle import oracle as o  # noqa: E402
from oracle import refimport  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "fusion_edges.npz")
SIGMA = 0.6
DIST_TH, DOT_TH = 0.0625, 0.5
f32 = np.float32
EYE = np.eye(4, dtype=f32)


def Kmat(fx, fy, cx, cy):
    return np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)


def palette(H, W):
    h, w = np.mgrid[0:H, 0:W]
    return np.stack([(h % 4) / 4.0, (w % 8) / 8.0, ((h + w) % 2) * 0.5 + 0.25], -1).astype(f32)


def up1(x):
    return np.nextafter(f32(x), f32(np.inf))


def dn1(x):
    return np.nextafter(f32(x), f32(-np.inf))


def hand_pixel(u, v, z, H, W):
    """Pixel of a camera-frame point whose image coordinates (u, v) are EXACT rationals: fusionutils.py:259-274 in
    rational arithmetic (bounds as the float32 values the comparison sees; round half to even)."""
    lo, uh, vh = Fraction(float(f32(-1e-3))), Fraction(float(f32(W - 0.999))), Fraction(float(f32(H - 0.999)))
    if not (z > 0 and lo < u < uh and lo < v < vh):
        return -1
    w, h = round(u), round(v)   # Python rounds a Fraction half to even
    return min(max(h, 0), H - 1) * W + min(max(w, 0), W - 1)


class Ref:
    """The reference's side of a scene."""

    def __init__(self):
        refimport.import_reference()
        import torch
        from gradslam.slam import fusionutils as fu
        from gradslam.structures.pointclouds import Pointclouds
        from gradslam.structures.rgbdimages import RGBDImages
        self.torch, self.fu, self.Pointclouds, self.RGBDImages = torch, fu, Pointclouds, RGBDImages

    def frames(self, fr):
        T = self.torch.from_numpy
        st = lambda k: T(np.stack([f[k] for f in fr]))   # noqa: E731
        return self.RGBDImages(st("rgb")[:, None], st("depth")[:, None, ..., None], st("K")[:, None], st("pose")[:, None])

    def maps(self, fr):
        """frame dict(depth, rgb, K, pose) -> the same dict with the reference's maps added"""
        r = self.frames([fr])
        al = self.fu.get_alpha(r.vertex_map, dim=4, keepdim=True, sigma=SIGMA)
        return dict(fr, vertex=r.vertex_map[0, 0].numpy(), normal=r.normal_map[0, 0].numpy(),
                    gvertex=r.global_vertex_map[0, 0].numpy(), gnormal=r.global_normal_map[0, 0].numpy(),
                    alpha=al[0, 0, ..., 0].numpy())

    def run(self, seqs, dist_th, dot_th):
        T, fu = self.torch.from_numpy, self.fu
        fr = self.frames(seqs)
        if all(s["P"].shape[0] == 0 for s in seqs):
            pc = self.Pointclouds()
        else:
            pc = self.Pointclouds(points=[T(s["P"].copy()) for s in seqs], normals=[T(s["N"].copy()) for s in seqs],
                                  colors=[T(s["C"].copy()) for s in seqs], features=[T(s["F"].copy()) for s in seqs])
        act = fu.find_active_map_points(pc, fr)
        sim, mask = fu.find_similar_map_points(pc, fr, act, dist_th, dot_th)
        uq = fu.find_best_unique_correspondences(pc, fr, sim)
        act, mask, uq = act.numpy(), mask.numpy(), uq.numpy()
        fused = fu.fuse_with_map(pc, fr, self.torch.from_numpy(uq), SIGMA)   # (mutates pc: nothing reads it afterwards)
        for b, s in enumerate(seqs):
            sel = act[:, 0] == b
            s["active"], s["similar_mask"], s["unique"] = fe.rows_of(act, b), mask[sel], fe.rows_of(uq, b)
            s["fP"], s["fN"] = fused.points_list[b].numpy().copy(), fused.normals_list[b].numpy().copy()
            s["fC"], s["fF"] = fused.colors_list[b].numpy().copy(), fused.features_list[b].numpy().copy()


def map_of(P, N=None, C=None, F=None, rng=None):
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    n = P.shape[0]
    N = np.tile(f32([0, 0, 1]), (n, 1)) if N is None else np.ascontiguousarray(np.asarray(N, f32).reshape(n, 3))
    if C is None:   # dyadic colours
        C = (np.arange(3 * n).reshape(n, 3) % 16 / 16.0).astype(f32)
    F = np.ones((n, 1), f32) if F is None else np.asarray(F, f32).reshape(n, 1).copy()
    return dict(P=P, N=N, C=np.ascontiguousarray(C, f32), F=F)


def exact_frame(H, W, f, depth=None, pose=EYE, K=None):
    K = Kmat(f, f, W // 2, H // 2) if K is None else K
    depth = np.ones((H, W), f32) if depth is None else depth
    return dict(depth=depth, rgb=palette(H, W), K=K, pose=pose)


def cam_point(u, v, z, K):
    """camera-frame point of image coordinates (u, v) at depth z (dyadic inputs: exact)"""
    return [(u - float(K[0, 2])) / float(K[0, 0]) * z, (v - float(K[1, 2])) / float(K[1, 1]) * z, z]


# ------------------------------------------------------------------------------------------------ the scenes
def scene_borders(ref):
    H, W = 5, 7
    fr = ref.maps(exact_frame(H, W, 4.0))
    K, e = fr["K"], 2.0 ** -10
    uvz = [(-e, 0, 1), (-2 * e, 0, 1), (1, -e, 1), (1, -2 * e, 1), (W - 1 + e, 1, 1), (W - 1 + 2 * e, 1, 1),
           (2, H - 1 + e, 1), (2, H - 1 + 2 * e, 1), (0.5, 3, 1), (1.5, 3, 1), (2.5, 3, 1), (3.5, 3, 1), (5, 0.5, 1),
           (5, 1.5, 1), (5, 2.5, 2), (4.5, 3.5, 0.5), (3, 2, 0.0), (3, 2, -1.0), (3, 2, 2.0 ** -20)]
    hand = [0, -1, 1, -1, 13, -1, 30, -1, 21, 23, 23, 25, 5, 19, 19, 32, -1, -1, 17]
    P = [cam_point(u, v, z, K) for u, v, z in uvz]
    P += [[0.25, 0.0, 2.0 ** -20], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]]   # u = 2^20 + 3; the origin, both signs
    hand += [-1, -1, -1]
    P.append(fr["gvertex"][1, 4].tolist())   # exactly a pixel's vertex
    hand.append(11)
    for (u, v, z), hp in zip(uvz, hand):   # the literals above against the rational formula
        if z > 0:
            assert hp == hand_pixel(Fraction(u), Fraction(v), z, H, W), (u, v, z, hp)
    return dict(H=H, W=W, seqs=[dict(fr, expect_pix=np.array(hand, np.int32), **map_of(P))])


def scene_borders_kzero(ref):
    """K's third row (0, 0, 1, -1): r[2] = z - 1 is 0 for a point at z = 1 -> the division by 1 (projutils.py)"""
    H, W = 5, 7
    K = Kmat(4.0, 4.0, 3.0, 2.0)
    K[2, 3] = -1.0
    fr = ref.maps(exact_frame(H, W, 4.0, K=K))
    # (x, y, z) -> r = (4x + 3z, 4y + 2z, z - 1)
    P = [[0, 0, 1], [0.75, 0.5, 1], [0, 0, 2], [0, 0, 0.5], [-0.5, 0.25, 2], [1.0, 0.5, 1]]
    hand = [17, 34, 34, -1, 32, -1]   # (3,2)/1; (6,4)/1; (6,4)/1; (1.5,1)/-0.5 < 0; (4,5)/1 -> v = 5 out... see below
    hand[4] = hand_pixel(Fraction(4), Fraction(5), 1, H, W)     # v = 5 >= H - 0.999: outside
    hand[5] = hand_pixel(Fraction(7), Fraction(4), 1, H, W)     # u = 7: outside
    assert hand[4] == -1 and hand[5] == -1
    return dict(H=H, W=W, seqs=[dict(fr, expect_pix=np.array(hand, np.int32), **map_of(P))])


def scene_borders_perm(ref):
    """32x64, pose = a 90 degree axis permutation with a dyadic translation, 1025 points on a quarter-pixel grid that
    overhangs the frame by a pixel on every side, depths 0.5 / 1 / 2: every k + 0.5 of the frame is hit"""
    H, W, n = 32, 64, 1025
    pose = np.array([[0, 0, 1, 0.5], [-1, 0, 0, -0.25], [0, -1, 0, 2.0], [0, 0, 0, 1]], f32)
    fr = ref.maps(exact_frame(H, W, 32.0, pose=pose))
    K, R, t = fr["K"], pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    rng = np.random.default_rng(21)
    P, hand = [], []
    for i in range(n):
        u = Fraction(int(rng.integers(-4, 4 * W + 1)), 4)
        v = Fraction(int(rng.integers(-4, 4 * H + 1)), 4)
        z = [0.5, 1.0, 2.0][i % 3]
        q = np.array(cam_point(float(u), float(v), z, K))
        P.append(R @ q + t)
        hand.append(hand_pixel(u, v, z, H, W))
    N = np.tile((R @ np.array([0, 0, 1.0])).astype(f32), (n, 1))
    F = np.array([0.5, 1.0, 1.0, 2.0], f32)[rng.integers(0, 4, n)]
    return dict(H=H, W=W, seqs=[dict(fr, expect_pix=np.array(hand, np.int32), **map_of(P, N=N, F=F))])


def general_frame(H, W, seed, xi, bad=False):
    rng = np.random.default_rng(seed)
    depth = (1.0 + np.round(rng.random((H, W)) * 32) / 16).astype(f32)
    depth[rng.random((H, W)) < 0.2] = 0
    depth[:, -1] = 0
    if H * W > 4096:   # (keeps the file small: depth in 8x8 patches, one in eight)
        h, w = np.mgrid[0:H, 0:W]
        depth[(h // 8 + w // 8) % 8 != 0] = 0
    if bad:
        depth[-1, :3] = [-1.0, np.nan, np.inf]
        depth[H // 2, W // 2] = np.inf
        depth[0, 1] = np.nan
    s = W / 131.0   # neg_fy_ragged's camera, scaled to the frame: non-square, negative fy
    K = np.array([[120.3 * s, 0, 65.2 * s, 0], [0, -120.0 * s, 0.5 * H - 0.4, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
    return dict(depth=depth, rgb=rng.integers(0, 16, (H, W, 3)).astype(f32) / f32(16), K=K,
                pose=o.se3_exp(np.asarray(xi, f32)))


def general_map(fr, n, seed, jitter=0.01):
    """n surfels near the frame's surface: pixels' global vertices (cycled), jittered; few confidence values, so that
    several rows compete for most pixels"""
    rng = np.random.default_rng(seed)
    valid = np.flatnonzero(np.isfinite(fr["depth"].ravel()) & (fr["depth"].ravel() > 0))
    idx = valid[rng.integers(0, valid.size, n)] if n else np.zeros(0, np.int64)
    P = fr["gvertex"].reshape(-1, 3)[idx] + (rng.standard_normal((n, 3)) * jitter).astype(f32)
    N = fr["gnormal"].reshape(-1, 3)[idx] + (rng.standard_normal((n, 3)) * 0.2).astype(f32)
    F = np.array([0.3, 0.7, 0.7, 1.9], f32)[rng.integers(0, 4, n)]   # (cc * x) * (1 / cc) is not the identity for these
    return map_of(P, N=N, C=rng.integers(0, 256, (n, 3)).astype(f32) / f32(256), F=F)


def scene_general(ref, H, W, n, seed, bad=False):
    fr = ref.maps(general_frame(H, W, seed, [0.1, -0.2, 0.05, 0.02, -0.01, 0.03], bad))
    return dict(H=H, W=W, seqs=[dict(fr, **general_map(fr, n, seed + 1))])


def scene_thresholds(ref, nodepth_dot=None):
    """All on the principal pixel (3, 2) of the exact 5x7 frame, whose global vertex is (0, 0, 1) and normal (0, 0, 1):
    distance exactly dist_th (rejected: the test is strict), one ulp below (accepted), dot exactly dot_th (rejected), one
    ulp above (accepted), non-unit normals.  The last row sits within dist_th of the world origin and projects onto pixel
    (0, 0), which has no depth (global vertex 0, normal 0)."""
    H, W = 5, 7
    depth = np.ones((H, W), f32)
    depth[0, 0] = 0
    fr = ref.maps(exact_frame(H, W, 4.0, depth=depth))
    assert fr["gvertex"][2, 3].tolist() == [0, 0, 1] and fr["gnormal"][2, 3].tolist() == [0, 0, 1]
    d, d1 = DIST_TH, float(dn1(DIST_TH))
    P = [[d, 0, 1], [d1, 0, 1], [0, d, 1], [0, d1, 1], [0, 0, 1 + d], [0, 0, 1 - d], [0.03125, 0, 1], [0.03125, 0, 1],
         [0.03125, 0, 1], [0.03125, 0, 1], [0.03125, 0, 1], [-0.0234375, -0.015625, 0.03125]]
    N = [[0, 0, 1]] * 6 + [[3, -4, 0.5], [0, 7, float(up1(0.5))], [0, 0, float(dn1(0.5))], [1, 1, 2], [0, 0, -1], [0, 0, 1]]
    accept = [0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0]   # by hand (the last one: the pixel's normal is 0, dot 0 < 0.5)
    hand = [17] * 11 + [0]
    hand[4] = hand_pixel(Fraction(3), Fraction(2), 1, H, W)
    sc = dict(H=H, W=W, seqs=[dict(fr, expect_pix=np.array(hand, np.int32), **map_of(P, N=N))], accept=accept)
    if nodepth_dot is not None:   # dot_th below 0: the depth-less pixel now matches (recorded as the reference does it)
        sc["dot_th"] = nodepth_dot
        sc["accept"] = [0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0, 1]   # (row 10: dot = -1 is not > -1)
    return sc


def tie_frame(ref):
    return ref.maps(exact_frame(32, 64, 32.0))


def scene_ties(ref, which):
    """32x64 exact frame, 2050 rows; every contested pixel has its rows in different 256-blocks.  Rows are the pixel's
    global vertex moved along x by dx (distance |dx|, 1/8 pixel at most).  Fillers: behind the camera, or in the frame
    with a normal that fails the test."""
    H, W, n = 32, 64, 2050
    fr = tie_frame(ref)
    gv = fr["gvertex"]
    P = np.zeros((n, 3), f32)
    P[:, 2] = -1.0                       # fillers behind the camera ...
    N = np.tile(f32([0, 0, 1]), (n, 1))
    F = np.ones(n, f32)
    for i in range(300, 600):            # ... and fillers on pixels of row 30, not similar
        P[i] = gv[30, i % W]
        N[i] = [0, 0, -1]
    win = {}

    def put(pix, rows, winner):
        h, w = pix
        for r, dx, cc, *rest in rows:
            P[r] = gv[h, w] + f32([dx, 0, 0])
            F[r] = cc
            if rest:
                N[r] = rest[0]
        win[h * W + w] = winner
    a, b, c = 2.0 ** -7, 2.0 ** -8, 2.0 ** -9
    if which in ("all", "none"):
        put((3, 5), [(3, a, 1), (700, b, 1)], 700)                      # equal confidence, different distance
        put((3, 9), [(4, a, 2), (701, c, 1)], 4)                        # higher confidence beats nearer
    if which in ("all", "one"):
        put((5, 40), [(705, b, 1), (5, b, 1)], 5)                       # bit-identical pair: the lower index
    if which == "all":
        put((7, 20), [(6, b, 1), (702, b, 1), (2049, b, 1)], 6)         # bit-identical triple
        put((9, 33), [(7, b, 1), (703, b, 1), (2048, b, 2)], 2048)      # pair + a strictly better key: spurious mark
        put((9, 50), [(8, b, 2), (704, b, 1), (2047, b, 1)], 8)         # the same with the better key first
        put((11, 12), [(9, b, 0.5), (706, b, 1), (2046, b, 1)], 706)    # pair + a lower-indexed row with a worse key
        put((13, 60), [(10, b, 1e20, [0, 0, -1]), (707, a, 1)], 707)    # the best key fails similarity
        put((15, 2), [(11, b, 0), (708, b, 1e-30), (2045, a, 1e20)], 2045)
        put((17, 31), [(12, a, 0), (709, b, 1e-30)], 709)               # 1/(cc + 1e-20) ties: the distance decides
        put((0, 0), [(13, b, 1), (1300, b, 1)], 13)                     # pixel 0 and pixel P - 1
        put((31, 63), [(2044, -b, 1), (14, -b, 1)], 14)
    best = np.full(H * W, -1, np.int32)
    for p, r in win.items():
        best[p] = r
    return dict(H=H, W=W, seqs=[dict(fr, **map_of(P, N=N, F=F))], expect_best=best)


def scene_merge(ref):
    """9x13 exact frame; one row per case, each alone on its pixel."""
    H, W = 9, 13
    fr = ref.maps(exact_frame(H, W, 8.0))
    gv, al = fr["gvertex"], fr["alpha"]
    pix = [(1, 1), (2, 3), (4, 6), (6, 2), (7, 11), (4, 9)]
    P = np.array([gv[h, w] for h, w in pix] + [[0, 0, -1.0], [-0.0, 0.0, -2.0]], f32)
    P[2] = [-0.0, -0.0, 1.0]                                    # -0.0 components, matched (the principal pixel)
    P[0, 0] += f32(2.0 ** -6)
    F = np.array([-al[1, 1], 0.0, 1.0, 1e-30, 1e20, 0.5, 1.0, 3.0], f32)   # cc + alpha == 0; cc = 0 with alpha > 0; ...
    C = np.array([[0.5, -0.0, 0.25]] * 8, f32)
    best = np.full(H * W, -1, np.int32)
    for r, (h, w) in enumerate(pix):
        best[h * W + w] = r
    return dict(H=H, W=W, seqs=[dict(fr, **map_of(P, C=C, F=F))], expect_best=best)


def scene_merge_nomatch(ref):
    """Rows in the frame, none similar: the merge is skipped, the rows keep their bits (-0.0 included)."""
    H, W = 9, 13
    fr = ref.maps(exact_frame(H, W, 8.0))
    P = fr["gvertex"].reshape(-1, 3)[::2] + f32([0, 0, 2.0 ** -8])
    P[0, :2] = -0.0
    n = P.shape[0]
    F = np.linspace(0.3, 1.7, n).astype(f32)   # (cc * x) * (1 / cc) would not be the identity for these
    return dict(H=H, W=W, seqs=[dict(fr, **map_of(P, N=np.tile(f32([0, 0, -1]), (n, 1)), F=F))],
                expect_best=np.full(H * W, -1, np.int32))


def scene_append(ref, H, W, f, keep_new, depth=None):
    """exact frame whose map is the global vertex of every valid pixel that is NOT in keep_new: exactly those are new"""
    fr = ref.maps(exact_frame(H, W, f, depth=depth))
    valid = np.flatnonzero(fr["depth"].ravel() > 0)
    rows = np.array([p for p in valid if p not in keep_new], np.int64)
    P = fr["gvertex"].reshape(-1, 3)[rows]
    best = np.full(H * W, -1, np.int32)
    best[rows] = np.arange(rows.size)
    return dict(H=H, W=W, seqs=[dict(fr, **map_of(P, N=fr["gnormal"].reshape(-1, 3)[rows]))], expect_best=best)


def scene_batch(ref, kind):
    """B sequences on 9x13 general frames with ragged map sizes."""
    H, W = 9, 13
    sizes = {"batch9": [257, 0, 1, 255, 256, 33, 300, 90, 351], "batch9_late": [20, 0, 1, 17, 30, 9, 64, 33, 120],
             "batch2_one_empty_table": [100, 257]}[kind]
    seqs = []
    for b, n in enumerate(sizes):
        fr = ref.maps(general_frame(H, W, 100 + b, [0.02 * b, -0.1, 0.05, 0.02, -0.01 * b, 0.03]))
        m = general_map(fr, n, 200 + b)
        last = b == len(sizes) - 1
        if n == 1:
            m["P"][0] = fr["pose"][:3, :3] @ f32([0, 0, -1]) + fr["pose"][:3, 3]      # behind the camera
        elif (kind == "batch9_late" and not last) or (kind == "batch2_one_empty_table" and b == 0) or (kind == "batch9" and b == 3):
            m["N"] = -m["N"]                                                           # in the frame, never similar
        seqs.append(dict(fr, **m))
    return dict(H=H, W=W, seqs=seqs)


def scene_tiny(ref, H, W):
    if H == 1:   # the reference cannot run it (see the module docstring): the oracle's maps, ref = 0
        depth, K = np.array([[2.0]], f32), Kmat(2.0, 2.0, 0.0, 0.0)
        v, n = np.array([[[0, 0, 2]]], f32), np.zeros((1, 1, 3), f32)   # (no neighbour to difference against: normal 0)
        fr = dict(depth=depth, rgb=palette(1, 1), K=K, pose=EYE, vertex=v, normal=n, gvertex=v, gnormal=n,
                  alpha=o.alpha(v, SIGMA))
        P = [[0, 0, 2], [0, 0, 2.03125], [2.0 ** -11, 0, 2], [2.0 ** -9, 0, 2], [1, 0, 2]]   # u = x: 2^-11 in, 2^-9 out
        return dict(H=1, W=1, seqs=[dict(fr, expect_pix=np.array([0, 0, 0, -1, -1], np.int32), **map_of(P))], ref=0,
                    dot_th=-1.0, expect_best=np.array([0], np.int32))
    fr = ref.maps(exact_frame(H, W, 2.0))
    P = np.concatenate([fr["gvertex"].reshape(-1, 3), fr["gvertex"].reshape(-1, 3)[:1]])
    return dict(H=H, W=W, seqs=[dict(fr, **map_of(P))])


def build_scenes(ref):
    sc = {}
    sc["borders"] = scene_borders(ref)
    sc["borders_kzero"] = scene_borders_kzero(ref)
    sc["borders_perm"] = scene_borders_perm(ref)
    sc["general_ragged"] = scene_general(ref, 67, 131, 1023, 31, bad=True)
    sc["general_dense"] = scene_general(ref, 13, 29, 3 * 13 * 29, 41)
    sc["thresholds"] = scene_thresholds(ref)
    sc["thresholds_nodepth"] = scene_thresholds(ref, nodepth_dot=-1.0)
    sc["ties"] = scene_ties(ref, "all")
    sc["ties_one_mark"] = scene_ties(ref, "one")
    sc["ties_no_mark"] = scene_ties(ref, "none")
    sc["merge"] = scene_merge(ref)
    sc["merge_nomatch"] = scene_merge_nomatch(ref)
    Pn = 67 * 131
    bad = np.ones((32, 64), f32)
    bad.ravel()[[0, 1, 2, 1023, 1024, 2047]] = [-1.0, np.nan, np.inf, np.inf, np.nan, -0.0]
    sc["append_all_new"] = dict(H=32, W=64, seqs=[dict(ref.maps(exact_frame(32, 64, 32.0, depth=bad)), **map_of(np.zeros((0, 3))))],
                                expect_best=np.full(2048, -1, np.int32))
    sc["append_none_new"] = scene_append(ref, 32, 64, 32.0, set())
    sparse = np.ones(Pn, f32)   # 67x131: the eight full tiles hold matched pixels and pixels without depth only
    sparse[:8192][(np.arange(8192) // 131) % 4 != 0] = 0   # (every fourth row: the normals stay defined)
    sc["append_last_tile"] = scene_append(ref, 67, 131, 64.0, set(range(8200, Pn, 3)), depth=sparse.reshape(67, 131))
    sc["append_first_only"] = scene_append(ref, 5, 7, 4.0, {0})
    sc["append_last_only"] = scene_append(ref, 5, 7, 4.0, {34})
    for k in ("batch9", "batch9_late", "batch2_one_empty_table"):
        sc[k] = scene_batch(ref, k)
    sc["tiny_1x1"] = scene_tiny(ref, 1, 1)
    sc["tiny_2x2"] = scene_tiny(ref, 2, 2)
    return sc


def main():
    ref = Ref()
    scenes = build_scenes(ref)
    out = {"scenes": np.array(list(scenes))}
    for name, sc in scenes.items():
        sc.update(name=name, B=len(sc["seqs"]), dist_th=sc.get("dist_th", DIST_TH), dot_th=sc.get("dot_th", DOT_TH))
        sc.setdefault("ref", 1)
        if sc["ref"]:
            ref.run(sc["seqs"], sc["dist_th"], sc["dot_th"])
        tabs = fe.oracle_scene(sc)
        if not sc["ref"]:
            for s, t in zip(sc["seqs"], tabs):
                s.update({k: t[k] for k in fe.OUT_FIELDS})
        fe.assert_oracle_is_reference(sc, tabs)          # the oracle reproduces the reference, or nothing is written
        for s in sc["seqs"]:                              # what the scene was constructed to show, by hand
            if "accept" in sc:
                assert s["similar_mask"].tolist() == [bool(a) for a in sc["accept"]], (name, s["similar_mask"])
            if "expect_best" in sc:
                assert np.array_equal(o.rows_to_best_pix(s["unique"], sc["H"], sc["W"]), sc["expect_best"]), name
                out[name + "/expect_best"] = sc["expect_best"]
        out[name + "/meta"] = np.array([sc["B"], sc["H"], sc["W"], sc["ref"]], np.int64)
        out[name + "/th"] = np.array([sc["dist_th"], sc["dot_th"]], np.float64)
        fields = fe.IN_FIELDS + fe.OUT_FIELDS + (("expect_pix",) if "expect_pix" in sc["seqs"][0] else ())
        for k in fields:   # one array per field: the sequences' arrays joined along axis 0, their lengths in /len
            out["%s/%s" % (name, k)] = np.concatenate([s[k] for s in sc["seqs"]], 0)
        out[name + "/len"] = np.array([[s[k].shape[0] for s in sc["seqs"]] for k in fields], np.int64)
        n_match = [int(s["unique"].shape[0]) for s in sc["seqs"]]
        print("%-24s B=%d %3dx%-3d maps %s matches %s new counts %s" % (
            name, sc["B"], sc["H"], sc["W"], [s["P"].shape[0] for s in sc["seqs"]], n_match,
            [s["fP"].shape[0] for s in sc["seqs"]]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "%.1f KiB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
