"""Pins the CPU oracle (oracle/gs_oracle.c) against golden vectors produced by the REAL
reference (oracle/make_golden.py).  Integer / index / mask outputs must be bit-exact; float
maps are bit-exact wherever the reference's arithmetic could be replicated operation by
operation (everything except exp() inside alpha, which is within 1 ulp).  CPU only."""
import math
import os

import numpy as np
import pytest

from oracle import oracle as o
from oracle import slam as oslam
from gradslam_amd.metrics import ate_rmse as ate

DIST_TH, DOT_TH, SIGMA = 0.05, math.cos(20 * math.pi / 180), 0.6


def ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_frame_maps_bit_exact(golden):
    g = golden("msrd_b0")
    for s in range(2):
        depth = g["depths"][s, ..., 0]
        v, n, a, valid = o.frame_maps(depth, g["intrinsics"], SIGMA)
        assert np.array_equal(v, g["vertex_map"][s])
        assert np.array_equal(n, g["normal_map"][s])
        assert np.array_equal(valid, depth > 0)
        gv, gn = o.global_maps(v, n, depth, g["poses"][s])
        assert np.array_equal(gv, g["global_vertex_map"][s])
        assert np.array_equal(gn, g["global_normal_map"][s])
        # alpha: exp() differs from torch's SLEEF exp by at most 1 ulp
        assert ulp_diff(a, g["alpha"][s]).max() <= 1
        np.testing.assert_allclose(a, g["alpha"][s], rtol=2e-7, atol=0)


def test_reference_tolerances_of_its_own_tests(golden):
    """tests/structures/test_rgbdimages.py:56-165 criteria, applied to the oracle."""
    g = golden("msrd_b0")
    v, n, _, _ = o.frame_maps(g["depths"][0, ..., 0], g["intrinsics"], SIGMA)
    assert ((g["vertex_map"][0] - v) ** 2).sum() < 1e-2
    assert (((g["normal_map"][0] - n) ** 2) < 1e-5).mean() >= 0.99


def test_first_frame_map(golden):
    g = golden("msrd_b0")
    depth = g["depths"][0, ..., 0]
    v, n, a, _ = o.frame_maps(depth, g["intrinsics"], SIGMA)
    gv, gn = o.global_maps(v, n, depth, g["poses"][0])
    e3, e1 = np.zeros((0, 3), np.float32), np.zeros((0, 1), np.float32)
    P, N, C, F = o.fuse_append(e3, e3, e3, e1, np.full(depth.size, -1, np.int32), gv, gn, g["colors"][0],
                               g["alpha"][0], depth)
    assert np.array_equal(P, g["map0_points"]) and np.array_equal(N, g["map0_normals"])
    assert np.array_equal(C, g["map0_colors"]) and np.array_equal(F, g["map0_ccounts"])


def test_correspondence_tables_bit_exact(golden):
    g = golden("msrd_b0")
    H, W = g["depths"].shape[1:3]
    P, N, F = g["map0_points"], g["map0_normals"], g["map0_ccounts"]
    gv1, gn1 = g["global_vertex_map"][1], g["global_normal_map"][1]
    pix = o.project_map(P, g["poses"][1], g["intrinsics"], H, W)
    act = o.active_table(pix, W)
    assert np.array_equal(act, g["active"])
    mask = o.similar_rows(act, P, N, gv1, gn1, DIST_TH, DOT_TH)
    assert np.array_equal(mask, g["similar_mask"])
    uq = o.best_unique_rows(act[mask], P, F, gv1)
    assert np.array_equal(uq, g["unique"])
    best, sim = o.associate(pix, P, N, F, gv1, gn1, DIST_TH, DOT_TH)
    assert np.array_equal(o.best_table(best, H, W), g["unique"])
    assert np.array_equal(o.rows_to_best_pix(g["unique"], H, W), best)
    assert sim.sum() == mask.sum()


def test_fuse_with_map_bit_exact(golden):
    g = golden("msrd_b0")
    H, W = g["depths"].shape[1:3]
    best = o.rows_to_best_pix(g["unique"], H, W)
    P, N, C, F = o.fuse_append(g["map0_points"], g["map0_normals"], g["map0_colors"], g["map0_ccounts"], best,
                               g["global_vertex_map"][1], g["global_normal_map"][1], g["colors"][1],
                               g["alpha"][1], g["depths"][1, ..., 0])
    for a, k in ((P, "points"), (N, "normals"), (C, "colors"), (F, "ccounts")):
        assert np.array_equal(a, g["map1_" + k]), k


def test_downsamplers(golden):
    g = golden("msrd_b0")
    p, n, _ = o.downsample_table(g["active"], 4, g["map0_points"], g["map0_normals"])
    assert np.array_equal(p, g["ds4_map_points"]) and np.array_equal(n, g["ds4_map_normals"])
    H, W = g["depths"].shape[1:3]
    pix = o.project_map(g["map0_points"], g["poses"][1], g["intrinsics"], H, W)
    p2, n2, _ = o.select_targets(pix, W, 4, g["map0_points"], g["map0_normals"])
    assert np.array_equal(p2, p) and np.array_equal(n2, n)
    fp, fn, _ = o.downsample_frame(g["global_vertex_map"][1], g["global_normal_map"][1], g["colors"][1],
                                   g["depths"][1, ..., 0], 4)
    assert np.array_equal(fp, g["ds4_frame_points"]) and np.array_equal(fn, g["ds4_frame_normals"])


def test_fusion_kat(golden):
    g = golden("fusion_kat")
    H, W = g["depth"].shape[:2]
    depth = g["depth"][..., 0]
    v, n, a, _ = o.frame_maps(depth, g["intrinsics"], float(g["sigma"]))
    gv, gn = o.global_maps(v, n, depth, g["pose"])
    uq = o.best_unique_rows(g["rows"], g["points"], g["ccounts"], gv)
    assert np.array_equal(uq, g["unique"])
    best = o.rows_to_best_pix(uq, H, W)
    P, N, C, F = o.fuse_append(g["points"], g["normals"], g["colors"], g["ccounts"], best, gv, gn, g["rgb"], a,
                               depth)
    assert P.shape == g["fused_points"].shape
    np.testing.assert_allclose(P, g["fused_points"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(N, g["fused_normals"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(C, g["fused_colors"], rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(F, g["fused_ccounts"], rtol=1e-6, atol=1e-9)
    P0, _, _, F0 = o.fuse_append(g["points"], g["normals"], g["colors"], g["ccounts"],
                                 np.full(H * W, -1, np.int32), gv, gn, g["rgb"], a, depth)
    np.testing.assert_allclose(P0, g["fused0_points"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(F0, g["fused0_ccounts"], rtol=1e-6, atol=1e-9)


def test_gauss_newton_and_solve(golden):
    g = golden("icp_unit")
    A, b, idx, keep = o.gauss_newton_rows(g["src"], g["tgt"], g["tgt_normals"])
    assert np.array_equal(idx, g["gn_idx"]) and keep.all()
    assert np.array_equal(A, g["gn_A"]) and np.array_equal(b, g["gn_b"][:, 0])
    A2, b2, idx2, keep2 = o.gauss_newton_rows(g["src"], g["tgt"], g["tgt_normals"], float(g["gn_thr"]))
    assert np.array_equal(idx2[keep2], g["gn_thr_idx"]) and np.array_equal(A2[keep2], g["gn_thr_A"])
    x = o.solve_normal_eq(A, b, 1e-8)
    np.testing.assert_allclose(x, g["solve_x"][:, 0], rtol=2e-3, atol=2e-6)


def test_se3_exp(golden):
    g = golden("icp_unit")
    for xi, T in zip(g["se3_xi"], g["se3_T"]):
        np.testing.assert_allclose(o.se3_exp(xi), T, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode,key", [(0, "icp"), (1, "gradicp")])
@pytest.mark.parametrize("iters", [3, 20])
def test_icp_transforms(golden, mode, key, iters):
    g = golden("icp_unit")
    T, idx = o.icp(g["src"], g["tgt"], g["tgt_normals"], mode=mode, numiters=iters)
    Tref = g["%s%d_T" % (key, iters)]
    np.testing.assert_allclose(T, Tref, rtol=0, atol=2e-5)
    assert (idx == g["%s%d_idx" % (key, iters)]).mean() > 0.995


@pytest.mark.parametrize("key,slam,odom", [("pf_gradicp", "pointfusion", "gradicp"), ("pf_icp", "pointfusion", "icp"),
                                           ("pf_gt", "pointfusion", "gt"), ("icpslam_gradicp", "icpslam", "gradicp")])
def test_sequences_64(golden, key, slam, odom):
    """Config C1 size: recovered poses within ATE 1e-4 m of the reference, identical map size."""
    g = golden("synth64")
    poses = g["poses"].copy()
    if odom != "gt":
        poses[1:] = poses[:1]
    m, rp = oslam.run_sequence(g["colors"], g["depths"], g["intrinsics"], poses, slam=slam, odom=odom)
    assert ate(rp, g[key + "_poses"]) <= 1e-4
    np.testing.assert_allclose(rp, g[key + "_poses"], rtol=0, atol=2e-5)
    assert len(m) == g[key + "_points"].shape[0]
    np.testing.assert_allclose(m.points, g[key + "_points"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(m.normals, g[key + "_normals"], rtol=1e-4, atol=1e-4)


def test_sequence_120(golden):
    g = golden("synth120")
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(4, 120, 160, seed=int(g["colors_seed"]))
    poses = g["poses"].copy()
    poses[1:] = poses[:1]
    m, rp = oslam.run_sequence(s["colors"], g["depths"], g["intrinsics"], poses)
    assert ate(rp, g["pf_gradicp_poses"]) <= 1e-4
    assert len(m) == int(g["pf_gradicp_count"])


def test_icpslam_640x480_first_frames(golden):
    """The oracle's ICPSLAM(odom="icp") frame loop against the REAL reference at the benchmarked resolution
    (tests/golden/icpslam640.npz, oracle/make_golden_640.py --slam icpslam): first 3 frames (the 8-frame run takes a
    minute on 8 cores and agrees to ATE 2e-6; the HIP path is compared with all 8 in tests/test_hip_batch.py)."""
    g = golden("icpslam640")
    from gradslam_amd.datasets.synthetic import make_sequence
    L = 3
    s = make_sequence(int(g["poses"].shape[0]), int(g["H"]), int(g["W"]), seed=int(g["seed"]))
    poses = s["poses"][:L].copy()
    poses[1:] = poses[:1]
    m, rp = oslam.run_sequence(s["colors"][:L], s["depths"][:L], s["intrinsics"][0], poses, slam="icpslam", odom="icp")
    assert ate(rp, g["poses"][:L]) <= 1e-5
    assert len(m) == int(g["counts"][L - 1])
    np.testing.assert_allclose(m.points.astype(np.float64).sum(0), g["sum_points"][L - 1], rtol=0, atol=1e-5 * len(m))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 7])
def test_pointfusion_640x480_first_frames_every_seed(golden, seed):
    """The oracle's PointFusion(odom="gradicp") frame loop against the REAL reference on each of the 8 sequences of the
    benchmark at 640x480 (tests/golden/pf640.npz, pf640_s1..7.npz, oracle/make_golden_640.py --seed): first 3 frames
    (5 s per seed here).  Poses within 1e-5 m ATE (measured 5e-7); the surfel counts differ by a handful of threshold
    flips -- poses that differ by ~1e-6 (float64 fixed-order sums here, float32 sgemm there) AND alpha that differs by
    1 ulp from torch's exp (test_pointfusion_640x480_ground_truth_odometry_vs_reference bounds that part on its own:
    <= 2 surfels over 8 frames with identical poses) --, bounded like the HIP test's."""
    g = golden("pf640" if seed == 0 else "pf640_s%d" % seed)
    from gradslam_amd.datasets.synthetic import make_sequence
    L = 3
    # (the first L frames: their depths are those of the golden's longer sequence, the colours differ and are not compared)
    s = make_sequence(L, int(g["H"]), int(g["W"]), seed=int(g["seed"]))
    assert int(g["seed"]) == seed
    poses = s["poses"][:L].copy()
    poses[1:] = poses[:1]
    m, rp = oslam.run_sequence(s["colors"][:L], s["depths"][:L], s["intrinsics"][0], poses)
    assert ate(rp, g["poses"][:L]) <= 1e-5
    diff = abs(len(m) - int(g["counts"][L - 1]))
    assert diff <= 5e-4 * int(g["counts"][L - 1])
    np.testing.assert_allclose(m.points.astype(np.float64).sum(0), g["sum_points"][L - 1], rtol=0,
                               atol=1e-5 * len(m) + 4.0 * diff + 1e-3)


@pytest.mark.parametrize("name", ["facets640_nh_l60", "facets640_l60", "pf640_l60"])
def test_long_horizon_goldens_first_frames(golden, name):
    """The long-horizon goldens of round 6.  tests/golden/<name>.npz is the REAL reference (oracle/make_golden_640.py),
    tests/golden/<name>_oracle.npz the oracle's trajectory over the same 60 frames (oracle/make_golden_oracle_long.py), which
    the HIP path must reproduce bit for bit over the whole horizon (tests/test_hip_batch.py).  Here, on the first 3 frames
    (seconds): the oracle golden is CURRENT (a fresh oracle run gives its bits: whoever changes the oracle regenerates it)
    and the oracle follows the reference to micrometres.
    facets640_nh_l60 is the scene the reference reproduces ITSELF on (inclined planes + ridge, no zeroed depth pixels: its
    3-thread run is within 4e-6 m of its 8-thread run over all 60 frames, reference_sensitivity_facets640_nh_l60.json) --
    the horizon on which BASELINE's ATE <= 1e-4 m is asserted against the reference; on the other two it drifts from itself
    (from frame 5 with zeroed pixels, from frame 28 on the benchmark scene) and the bound is derived from that drift."""
    import json
    from gradslam_amd.datasets.synthetic import make_sequence
    g, og = golden(name), golden(name + "_oracle")
    L, H, W = 3, int(g["H"]), int(g["W"])
    scene = str(g["scene"]) if "scene" in g.files else "wave"
    hole = float(g["hole_frac"]) if "hole_frac" in g.files else 0.05
    # (only the frames that are used: the depths of frame f do not depend on the length of the sequence, the colours do --
    # and nothing compared here depends on the colours; the GPU test checks the checksum of all 60 depth frames)
    s = make_sequence(L, H, W, seed=int(g["seed"]), scene=scene, hole_frac=hole)
    poses = s["poses"][:L].copy()
    poses[1:] = poses[:1]
    counts = []
    m, rp = oslam.run_sequence(s["colors"][:L], s["depths"][:L], s["intrinsics"][0], poses, per_frame=lambda f, mm, p: counts.append(len(mm)))
    assert np.array_equal(rp.astype(np.float32).view(np.int32), og["poses"][:L].view(np.int32))
    assert counts == [int(x) for x in og["counts"][:L]]
    assert ate(rp, g["poses"][:L]) <= 1e-5
    assert counts[0] == int(g["counts"][0]) and abs(counts[-1] - int(g["counts"][L - 1])) <= 5e-4 * int(g["counts"][L - 1])
    # the oracle golden against the reference golden over the WHOLE horizon, as far as the reference reproduces itself
    d = np.linalg.norm(og["poses"][:, :3, 3].astype(np.float64) - g["poses"][:, :3, 3], axis=1)
    if name == "facets640_nh_l60":
        with open(os.path.join(os.path.dirname(__file__), "golden", "reference_sensitivity_facets640_nh_l60.json")) as fh:
            sens = json.load(fh)
        assert max(sens["translation_diff_per_frame_m"]) <= 1e-5          # the gate: the reference agrees with itself
        assert float(np.sqrt((d * d).mean())) <= 1e-4 and d.max() <= 1e-4, d.max()   # BASELINE's bound, all 60 frames
    else:
        calm = 28 if name == "pf640_l60" else 5
        assert d[:calm].max() <= 5e-5, d[:calm].max()


def test_pointfusion_640x480_ground_truth_odometry_vs_reference(golden):
    """The fusion path (K5 association, K6 merge + append) across 8 frames at the benchmarked size with NO ICP in the
    loop: the oracle's PointFusion(odom="gt") against the REAL reference (tests/golden/pf640_gt.npz,
    oracle/make_golden_640.py --odom gt).  The first map is exact (sha256 of its tables); from the second frame on the
    confidence counts carry alpha, and torch's exp (MKL VML on this build, not restatable) is 1 ulp away from the
    specified polynomial on ~10 % of the pixels, so a merge near a threshold can go the other way: measured, the surfel
    counts stay identical for 6 frames and differ by 1 / 2 of 5.4e5 / 5.7e5 afterwards; attribute sums per surfel agree
    to 7e-6 m (points), 4e-6 (normals), 6e-4 of 255 (colours), 2e-11 (confidence counts).  This is the part of the
    per-frame drift of the gradICP runs that does NOT come from the poses."""
    import hashlib
    from gradslam_amd.datasets.synthetic import make_sequence
    g = golden("pf640_gt")
    L, H, W = int(g["poses"].shape[0]), int(g["H"]), int(g["W"])
    s = make_sequence(L, H, W, seed=int(g["seed"]))
    assert abs(float(s["depths"].astype(np.float64).sum()) - float(g["depth_sum"])) < 1e-6 * float(g["depth_sum"])
    assert np.array_equal(g["poses"], s["poses"])            # ground-truth odometry hands the frames' poses through
    rec = []

    def per(f, m, pose):
        if f == 0:
            rec.append([hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in (m.points, m.normals, m.colors)])
        rec.append((len(m), m.points.astype(np.float64).sum(0), m.normals.astype(np.float64).sum(0),
                    m.colors.astype(np.float64).sum(0), m.ccounts.astype(np.float64).sum(0)))

    oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gt", per_frame=per)
    assert rec[0] == [str(x) for x in g["sha_frame0"]]
    rec = rec[1:]
    for f in range(L):
        n, sp, sn, sc, scc = rec[f]
        assert abs(n - int(g["counts"][f])) <= (0 if f < 4 else 3), (f, n, int(g["counts"][f]))
        for mine, ref, tol in ((sp, g["sum_points"][f], 2e-5), (sn, g["sum_normals"][f], 1e-5),
                               (sc, g["sum_colors"][f], 2e-3), (scc, g["sum_ccounts"][f], 1e-9)):
            assert np.abs(mine - ref).max() <= tol * n + 4.0 * abs(n - int(g["counts"][f])) * (255.0 if tol == 2e-3 else 3.0), (f, tol)


def test_relative_pose_matches_reference(golden):
    """gs_or_relative_pose against GroundTruthOdometryProvider / relative_transformation of the reference
    (torch.inverse in float32 there, double Gauss-Jordan here: equal to a few float32 ulps)."""
    g = golden("gt_odom")
    rel = o.relative_pose(g["T1"], g["T2"])
    assert np.abs(rel - g["rel"][:, 0]).max() <= 2e-6
    assert np.array_equal(rel[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (rel.shape[0], 1)))


def test_fuse_adjoint_by_finite_differences():
    """oracle/fusion_backward.py: the reverse mode of merge + append against central differences of its own
    float64 forward (matched, unmatched and zero-confidence rows, appended pixels)."""
    from oracle import fusion_backward as fb
    rng = np.random.default_rng(0)
    n, P = 12, 20
    old = [rng.standard_normal((n, 3)) for _ in range(3)]
    cc = rng.random(n) + 0.1
    cc[3] = 0.0
    frame = [rng.standard_normal((P, 3)) for _ in range(3)]
    alpha = rng.random(P)
    pix_of = np.full(n, -1)
    pix_of[[0, 2, 3, 5, 9]] = [4, 7, 1, 15, 11]
    new_pix = np.array([0, 2, 3, 8, 19])
    W = [rng.standard_normal((n + len(new_pix), 3)) for _ in range(3)]
    Wc = rng.standard_normal(n + len(new_pix))

    def loss(old, cc, frame, alpha):
        out, c2 = fb.fuse_forward(old, cc, frame, alpha, pix_of, new_pix)
        return sum((o_ * w).sum() for o_, w in zip(out, W)) + (c2 * Wc).sum()

    ob, cb, fbar, ab = fb.fuse_backward(old, cc, frame, alpha, pix_of, new_pix, W, Wc)
    h = 1e-6

    def fd(arr, idx, rebuild):
        e = np.zeros_like(arr)
        e[idx] = h
        return (rebuild(arr + e) - rebuild(arr - e)) / (2 * h)
    for t in range(3):
        for idx in ((0, 1), (3, 0), (7, 2)):
            assert abs(fd(old[t], idx, lambda v: loss([v if k == t else old[k] for k in range(3)], cc, frame, alpha))
                       - ob[t][idx]) < 1e-6
        for idx in ((4, 0), (1, 2), (8, 1), (5, 0)):
            assert abs(fd(frame[t], idx, lambda v: loss(old, cc, [v if k == t else frame[k] for k in range(3)], alpha))
                       - fbar[t][idx]) < 1e-6
    for i in (0, 1, 5):      # (row 3 has cc' = alpha != 0 here; a zero cc' row has a zero derivative by the guard)
        assert abs(fd(cc, i, lambda v: loss(old, v, frame, alpha)) - cb[i]) < 1e-6
    for p in (4, 7, 1, 0, 19, 6):
        assert abs(fd(alpha, p, lambda v: loss(old, cc, frame, v)) - ab[p]) < 1e-6


def test_frame_maps_adjoint_matches_reference_autograd(golden):
    """oracle/maps_backward.py (float64 numpy reverse mode of depth -> vertex, normal, alpha) against the
    reference's autograd (depth_grad.npz); the reference's float32 normal normalisation is noisy on a few
    near-degenerate pixels, so the comparison is robust (same criterion as the GPU test)."""
    from oracle import maps_backward as mb
    g = golden("depth_grad")
    got = mb.frame_maps_backward(g["depths"][1, ..., 0], g["intrinsics"], 0.6, g["Wv"], g["Wn"], g["Wa"])
    ref = g["maps_depth_grad"]
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and np.median(err) < 1e-4 * np.abs(ref).max()
    assert (err < 1e-2 * np.abs(ref).max()).mean() > 0.999


def test_intrinsics_adjoint_matches_reference_autograd(golden):
    """oracle/maps_backward.py K_bar against the reference's autograd d/dK (tests/golden/intrinsics_grad.npz)."""
    from oracle import maps_backward as mb
    g, gk = golden("depth_grad"), golden("intrinsics_grad")
    d_bar, K_bar = mb.frame_maps_backward(gk["depth"], gk["intrinsics"], 0.6, g["Wv"], g["Wn"], g["Wa"], want_K=True)
    ref = gk["K_grad"]
    assert np.array_equal(K_bar == 0, ref == 0)
    assert np.abs(K_bar - ref).max() <= 1e-4 * np.abs(ref).max(), (K_bar, ref)
    assert np.abs(d_bar - gk["depth_grad"]).max() <= 1e-3 * np.abs(gk["depth_grad"]).max()


def test_resize_known_answers_with_border_clamps():
    """OpenCV is not installed here, so the resize arithmetic of the dataset ingest (oracle.ingest_* and, bit for bit
    equal to it, gs_ingest_*: tests/test_hip_api.py) cannot be pinned against cv2 itself (PARITY UNPINNED for resized
    frames).  These are hand-computed answers of cv2.resize's documented conventions: INTER_LINEAR samples
    at (dst + 0.5) * scale - 0.5 and clamps at the borders; INTER_NEAREST takes floor(dst * scale)."""
    from oracle import oracle as o
    src = np.zeros((2, 2, 3), np.uint8)
    src[..., 0] = [[0, 10], [20, 30]]
    src[..., 1] = 255 - src[..., 0]
    up = o.ingest_color(src, 4, 4)
    want = np.array([[0, 2.5, 7.5, 10], [5, 7.5, 12.5, 15], [15, 17.5, 22.5, 25], [20, 22.5, 27.5, 30]], np.float32)
    assert np.array_equal(up[..., 0], want) and np.array_equal(up[..., 1], 255 - want) and not up[..., 2].any()
    # 4 -> 2: sample positions 0.5 and 2.5: the mean of the two neighbours
    row = np.zeros((1, 4, 3), np.uint8)
    row[0, :, 0] = [0, 10, 20, 40]
    assert np.array_equal(o.ingest_color(row, 1, 2)[0, :, 0], np.array([5.0, 30.0], np.float32))
    # 3 -> 2 (non-integer ratio 1.5): positions 0.25 and 1.75
    r3 = np.zeros((1, 3, 3), np.uint8)
    r3[0, :, 0] = [0, 100, 200]
    assert np.allclose(o.ingest_color(r3, 1, 2)[0, :, 0], [25.0, 175.0], atol=1e-4)
    assert np.array_equal(o.ingest_color(src, 2, 2, normalize=True)[..., 0], want[::3, ::3] / np.float32(255))
    d = np.array([[1000, 2000, 3000], [4000, 5000, 6000]], np.uint16)
    assert np.array_equal(o.ingest_depth(d, 2, 3, 1000.0), d.astype(np.float32) / 1000)
    assert np.array_equal(o.ingest_depth(d, 4, 6, 1000.0)[::2, ::2], d.astype(np.float32) / 1000)   # floor(dst / 2)
    assert np.array_equal(o.ingest_depth(d, 4, 6, 1000.0)[1::2, 1::2], d.astype(np.float32) / 1000)
    assert np.array_equal(o.ingest_depth(d, 1, 2, 5000.0), np.array([[0.2, 0.4]], np.float32))      # floor(dst * 1.5)


def test_validity_mask_can_be_read_off_the_local_vertex():
    """The fused step does not store the live frame's global maps; where the map update needs the global vertex of a pixel
    it transforms the local one and re-masks it with `vertex.z > 0` instead of `depth > 0` (gs_fuse.hip: FrameLocalMaps --
    one scattered access less per surfel).  That is the same mask for a vertex map made by the frame-map arithmetic
    (rgbdimages.py:643-679: z = (1 * d) * [d > 0]), whatever the depth holds: zeros, negatives, NaN, infinities,
    denormals, and whatever the intrinsics are."""
    rng = np.random.default_rng(5)
    H, W = 12, 16
    depth = rng.uniform(0.3, 4.0, (H, W)).astype(np.float32)
    special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-38, 3.4e38], np.float32)
    depth.reshape(-1)[:special.size * 3] = np.tile(special, 3)
    rng.shuffle(depth.reshape(-1))
    for K in (np.array([[525, 0, 8.5, 0], [0, 525, 6.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32),
              np.array([[-3.25, 0, 100.0, 0], [0, -120.0, -59.9, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)):
        with np.errstate(all="ignore"):
            v, n, a, valid = o.frame_maps(depth, K, 0.6)
            assert np.array_equal(v[..., 2] > 0, depth > 0) and np.array_equal(valid, depth > 0)
            # ... and the global vertex re-masked either way has the same bits
            pose = np.eye(4, dtype=np.float32)
            pose[:3, 3] = (0.3, -0.2, 0.1)
            gv, _ = o.global_maps(v, n, depth, pose)
            gz, _ = o.global_maps(v, n, np.where(v[..., 2] > 0, np.float32(1), np.float32(0)), pose)
        assert np.array_equal(gv.view(np.int32), gz.view(np.int32))


@pytest.mark.skipif(os.environ.get("GRADSLAM_SLOW_TESTS") != "1",
                    reason="minutes of CPU (60 frames of the oracle at 640x480): GRADSLAM_SLOW_TESTS=1; numbers of the "
                           "run in the build container are on record in DESIGN.md section 2")
def test_pointfusion_640x480_sixty_frames_oracle_vs_reference():
    """VERDICT r04 #5, CPU half: the oracle's frame loop against the REAL reference over the long horizon
    (tests/golden/pf640_l60.npz, 60 frames of sequence 0, oracle/make_golden_640.py --frames 60 --tag pf640_l60) -- the
    window in which every second solve wanders (frames 38 - 44) and the map grows to 1.4 M surfels.  ATE <= 1e-4 m, every
    pose within 1e-4, count drift within the bound the GPU test asserts."""
    import json
    from gradslam_amd import metrics as M
    from gradslam_amd.datasets.synthetic import make_sequence
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "pf640_l60.npz"))
    L = int(g["poses"].shape[0])
    s = make_sequence(L, 480, 640, seed=0)
    poses = s["poses"].copy()
    poses[1:] = poses[:1]
    counts = []
    m, rp = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], poses, per_frame=lambda f, mm, p: counts.append(len(mm)))
    a, d = M.ate_rmse(rp, g["poses"]), M.count_drift(counts, g["counts"])
    out = os.environ.get("GRADSLAM_TEST_RECORD")
    if out:
        with open(os.path.join(out, "long_horizon_oracle_pf640_l60.json"), "w") as fh:
            json.dump({"ate_m": a, "rpe": M.rpe(rp, g["poses"]), "count_drift": d}, fh)
    # (measured in the build container: frames 0 .. 27 ATE ~1e-6; from frame 28 on the reference's own solves no longer
    # settle within their 20 iterations and the two roundings of that iteration end up millimetres apart -- whole-horizon
    # ATE 2.76e-3 m, bit for bit what the HIP path gives: tests/test_hip_batch.py::test_pointfusion_long_horizon_...)
    c = 28
    assert M.ate_rmse(rp[:c], g["poses"][:c]) <= 1e-5
    np.testing.assert_allclose(rp[:c], g["poses"][:c], rtol=0, atol=1e-4)
    assert max(d["per_frame"][:c]) <= 300, d
    assert a <= 6e-3 and np.abs(rp - g["poses"]).max() <= 1.2e-2, a


@pytest.mark.parametrize("scene,b", [("ragged2", 0), ("ragged2", 1), ("hard3", 0)])
def test_engine_matrix_fixtures_reproduce(scene, b):
    """The oracle records of the ICP engine matrix (tests/golden/engine_<scene>_oracle.npz, oracle/make_golden_engine.py)
    are what the oracle computes now, bit for bit: a stale fixture would hold the GPU tests to the wrong numbers.  Both
    sequences of the ragged lattice and the first of the hard frames (~15 s of CPU)."""
    from oracle import make_golden_engine as mge
    g = np.load(mge.golden_path(scene))
    c = mge.SCENES[scene]
    assert (int(g["H"]), int(g["W"]), int(g["L"]), int(g["first"])) == (c["H"], c["W"], c["L"], c["first"])
    assert g["seeds"].tolist() == c["seeds"]
    r = mge.run_one(scene, b)
    assert r["depth_sum"] == float(g["depth_sum"][b])
    assert np.array_equal(r["poses"].view(np.int32), g["poses"][b].view(np.int32))
    assert np.array_equal(r["counts"], g["counts"][b])
    assert np.array_equal(r["sum_points"], g["sum_points"][b])
    assert np.array_equal(r["sample_idx"], g["sample_idx"][b])
    assert np.array_equal(r["sample_points"].view(np.int32), g["sample_points"][b].view(np.int32))
