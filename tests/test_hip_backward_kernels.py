"""Every hand-written backward kernel (config C3) alone against its float64 numpy adjoint, per element over ALL
elements, at ragged sizes and on the branches the end-to-end gradient tests never reach.

Kernels are called through gradslam_amd.ops (the *Function.apply classes, ops.icp_with_tape / ops.icp_backward), never
through a SLAM driver: a failure names one kernel.  Outputs that are pure copies or exact zeros are compared by bits.

Tolerances
  ICP   rel < 2e-4 against oracle/icp_backward.py, 5e-4 against the reference's autograd (the bars of
        tests/test_icp_backward.py); the oracle differentiates the tape the HIP forward recorded, so a difference is the
        backward kernel's.
  fuse  rel < 1e-5 against oracle/fusion_backward.py (the bar of test_hip_fuse_backward_matches_oracle).
  frame maps, global maps, pose sums, alpha: KERNEL_FACTOR x the float32-numpy-against-float64-numpy gap of the same
        adjoint on the very input of the case, at least FLOOR_ULPS float32 ulps (tests/backward_cases.py holds the
        measured gaps; tests/test_backward_oracles_cpu.py recomputes them).
`rel` is the largest error over all elements relative to the largest element of the oracle's result."""
import os

import numpy as np
import pytest
import torch

from oracle import fusion_backward as fb
from oracle import icp_backward as ib
from oracle import maps_backward as mb
from tests import backward_cases as bc

pytestmark = pytest.mark.gpu

ICP_ORACLE_BAR, ICP_REFERENCE_BAR, FUSE_BAR = 2e-4, 5e-4, 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gradslam_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def within(tag, got, ref, bound):
    """prints the figure, then asserts it: every element, relative to the largest element of the oracle"""
    err = bc.rel_err(got, ref)
    print("%-44s rel %.3e  bound %.3e" % (tag, err, bound))
    assert np.isfinite(got).all(), tag
    assert err <= bound, (tag, err, bound, np.unravel_index(np.abs(got - ref).argmax(), np.shape(ref)))


# ------------------------------------------------------------------------------------------------ frame maps
@pytest.mark.parametrize("loss", bc.FRAME_LOSSES)
@pytest.mark.parametrize("fy,scale", bc.FRAME_VARIANTS)
@pytest.mark.parametrize("H,W", bc.FRAME_SIZES)
def test_frame_maps_backward_per_pixel(ops, H, W, fy, scale, loss):
    """gs_frame_maps_backward_f32 (difference, depth and K-bar kernels): depth_bar of every pixel and K_bar, with and
    without the other gradient requested.  Sizes whose pixel count is not a multiple of the block, two-pixel-wide and
    two-pixel-high images, negative fy, both sides of the alpha clamp, loss through one map at a time."""
    depth, K = bc.frame_case(H, W, fy, scale)
    vb, nb, ab = bc.frame_weights(H, W, loss)
    ref_d, ref_K = mb.frame_maps_backward(depth, K, bc.SIGMA, vb, nb, ab, want_K=True)
    key = bc.frame_key(H, W, fy, scale, loss)
    gap_d, gap_K = bc.FRAME_GAP[key]
    for want in ("depth", "depth+K", "K"):
        d = dev(depth).requires_grad_("depth" in want)
        Kt = dev(K).requires_grad_("K" in want)
        v, n, a = ops.FrameMapsFunction.apply(d, Kt, bc.SIGMA)
        terms = [(m * dev(w)).sum() for m, w, c in ((v, vb, "v"), (n, nb, "n"), (a, ab, "a")) if c in loss]
        sum(terms).backward()
        if "depth" in want:
            got = host(d.grad)
            assert np.all(got[depth <= 0] == 0), "pixels without depth carry no gradient"
            if loss == "a":   # through alpha alone the zeros are structural: masked pixels and the clamp
                assert np.array_equal(got != 0, ref_d != 0), "a clamped alpha carries no gradient, any other does"
            within(key + " depth_bar [" + want + "]", got, ref_d, bc.kernel_bound(gap_d))
        else:
            assert d.grad is None
        if "K" in want:
            got = host(Kt.grad)
            mask = np.zeros((4, 4), bool)
            mask[0, 0] = mask[0, 2] = mask[1, 1] = mask[1, 2] = True
            assert np.all(got[~mask] == 0), "only fx, fy, cx, cy carry a gradient"
            within(key + " K_bar [" + want + "]", got, ref_K, bc.kernel_bound(gap_K))
        else:
            assert Kt.grad is None


# ------------------------------------------------------------------------------------------------ global maps / pose
@pytest.mark.parametrize("loss", bc.GLOBAL_LOSSES)
@pytest.mark.parametrize("H,W", bc.FRAME_SIZES)
def test_global_maps_and_pose_backward_alone(ops, H, W, loss):
    """gs_global_maps_backward_f32 and gs_global_maps_pose_backward_f32 on their own: ragged pixel counts (a tail block in
    the 12-sum reduction), gv_bar without gn_bar and the reverse."""
    depth, K = bc.frame_case(H, W)
    v, n = bc.local_maps(depth, K)
    pose = bc.generic_pose()
    gvb = bc.weights((H, W, 3), 4) if "gv" in loss else None
    gnb = bc.weights((H, W, 3), 5) if "gn" in loss else None
    ref_v, ref_n, ref_p = mb.global_maps_backward(v, n, depth, pose, gvb, gnb)
    key = "%dx%d/%s" % (H, W, loss)
    gap_v, gap_n, gap_p = bc.GLOBAL_GAP[key]
    vt, nt, pt = (dev(x).requires_grad_(True) for x in (v, n, pose))
    gv, gn = ops.GlobalMapsFunction.apply(vt, nt, dev(depth), pt)
    sum((m * dev(w)).sum() for m, w in ((gv, gvb), (gn, gnb)) if w is not None).backward()
    got_v, got_n, got_p = host(vt.grad), host(nt.grad), host(pt.grad)
    if ref_v is None:
        assert np.all(got_v == 0)
    else:
        assert np.all(got_v[depth <= 0] == 0), "invalid pixels are masked out of gvertex"
        within(key + " v_bar", got_v, ref_v, bc.kernel_bound(gap_v))
    if ref_n is None:
        assert np.all(got_n == 0)
    else:
        within(key + " n_bar", got_n, ref_n, bc.kernel_bound(gap_n))
    assert np.all(got_p[3] == 0), "the bottom row of the pose is a constant"
    within(key + " pose_bar", got_p, ref_p, bc.kernel_bound(gap_p))


# ------------------------------------------------------------------------------------------------ down-sampler
@pytest.mark.parametrize("ds", [1, 2, 4, 5])
@pytest.mark.parametrize("H,W", [(67, 131), (480, 640)])
def test_downsample_backward_is_an_exact_scatter(ops, H, W, ds):
    """gs_downsample_frame_backward_f32 alone: H, W not divisible by ds, ds = 1, invalid lattice pixels; copies, so bits."""
    depth, _ = bc.frame_case(H, W)
    lat = np.zeros((H, W), bool)
    lat[::ds, ::ds] = True
    assert (lat & (depth <= 0)).any()
    g = bc.weights((H, W, 3), 7)
    gt = dev(g).requires_grad_(True)
    pts = ops.DownsampleFramePointsFunction.apply(gt, dev(depth), ds)
    assert np.array_equal(bits(host(pts)), bits(mb.downsample_forward(g, depth, ds)))
    pb = bc.weights(tuple(pts.shape), 8)
    (pts * dev(pb)).sum().backward()
    ref = mb.downsample_backward(pb, depth, ds)
    got = host(gt.grad)
    assert np.array_equal(got != 0, ref != 0) and np.array_equal(bits(got), bits(ref))


# ------------------------------------------------------------------------------------------------ alpha
@pytest.mark.parametrize("n", bc.ALPHA_SIZES)
def test_alpha_backward_across_block_borders(ops, n):
    """gs_alpha_backward_f32: n on both sides of a block border and far beyond one block, points on both sides of the
    clamp; the point gradients and the sigma gradient (a sum over every block)."""
    p, ab = bc.alpha_points(n), bc.weights((n,), 6)
    ref_p, ref_s = mb.alpha_backward(p, bc.SIGMA, 1e-7, ab)
    assert (ref_p == 0).all(1).any() and (ref_p != 0).all(1).any()
    gap_p, gap_s = bc.ALPHA_GAP[n]
    pt = dev(p).requires_grad_(True)
    sigma = torch.tensor(bc.SIGMA, dtype=torch.float64, requires_grad=True)
    a = ops.AlphaFunction.apply(pt, sigma, 1e-7)
    (a * dev(ab)).sum().backward()
    got = host(pt.grad)
    assert np.all(got[(ref_p == 0).all(1)] == 0), "clamped points carry no gradient"
    within("alpha n=%d points_bar" % n, got, ref_p, bc.kernel_bound(gap_p))
    within("alpha n=%d sigma_bar" % n, np.array([float(sigma.grad)]), np.array([float(ref_s)]), bc.kernel_bound(gap_s))


# ------------------------------------------------------------------------------------------------ fuse
FUSE_FRAMES = [(6, 8), (67, 131), (480, 640)]
FUSE_N_OLD = [0, 1, 255, 256, 257, 70001]
FUSE_CASES = [(H, W, n_old, pattern, renorm)
              for H, W in FUSE_FRAMES for n_old in FUSE_N_OLD for pattern in ("some", "none", "all")
              for renorm in (False, True)
              if not (n_old == 0 and pattern != "none")          # nothing to match
              and not (pattern == "all" and n_old < H * W)]      # "every pixel matched" needs a row per pixel


def fuse_case(H, W, n_old, pattern):
    """Old map rows, frame maps and a one-to-one correspondence table.
    some: half of min(n_old, valid pixels) rows matched, the rows next to the block borders (0, 255, 256, 257, last)
          among them; the first matched row has ccount = 0 and its pixel alpha = 0, the second ccount = -alpha (both
          cc + alpha == 0); the first unmatched row has ccount = 0
    none: empty table (the identity branch);  all: every valid pixel matched, no appended row.
    A tenth of the pixels is invalid (zero or negative depth); invalid pixels are never matched and never appended."""
    rng = np.random.default_rng([H, W, n_old, len(pattern)])
    P = H * W
    old = [rng.standard_normal((n_old, 3)).astype(np.float32) for _ in range(3)]
    cc = (rng.random((n_old, 1)) + 0.2).astype(np.float32)
    frame = [rng.standard_normal((H, W, 3)).astype(np.float32) for _ in range(3)]
    alpha = rng.random((H, W)).astype(np.float32)
    depth = (rng.random((H, W)) + 0.5).astype(np.float32)
    bad = rng.random((H, W))
    depth[bad < 0.05] = 0.0
    depth[(bad >= 0.05) & (bad < 0.1)] *= -1.0
    vp = np.flatnonzero(depth.reshape(-1) > 0)
    m = {"none": 0, "all": len(vp), "some": max(1, min(n_old, len(vp)) // 2) if n_old else 0}[pattern]
    border = [r for r in (0, 255, 256, 257, n_old - 1) if 0 <= r < n_old]
    border = list(dict.fromkeys(border))[:m]
    rest = np.setdiff1d(np.arange(n_old), border)
    rows = np.concatenate([np.array(border, int), rng.choice(rest, m - len(border), replace=False)]).astype(int)
    pixs = rng.choice(vp, m, replace=False)
    best = np.full(P, -1, np.int32)
    best[pixs] = rows
    if m:
        cc[rows[0], 0] = 0.0
        alpha.reshape(-1)[pixs[0]] = 0.0
    if m > 1:   # cc + alpha == 0 with cc != 0: the numerator cc x + alpha f is not zero, so the guard on 1 / cc' matters
        cc[rows[1], 0] = -alpha.reshape(-1)[pixs[1]]
    pix_of = np.full(n_old, -1)
    pix_of[rows] = pixs
    if (pix_of < 0).any():   # an unmatched zero-confidence row: rewritten to zero by renorm_all, untouched without it
        cc[np.flatnonzero(pix_of < 0)[0], 0] = 0.0
    new_pix = np.flatnonzero((depth.reshape(-1) > 0) & (best < 0))
    return old, cc, frame, alpha, depth, best, pix_of, new_pix


@pytest.mark.parametrize("H,W,n_old,pattern,renorm", FUSE_CASES)
def test_fuse_append_backward_every_branch(ops, H, W, n_old, pattern, renorm):
    """gs_fuse_append_backward_f32: renorm_all False and True, the no-match identity branch, cc + alpha == 0, n_old = 0,
    no appended row, rows across block borders and many blocks, more than one compaction tile of pixels."""
    old, cc, frame, alpha, depth, best, pix_of, new_pix = fuse_case(H, W, n_old, pattern)
    P = H * W
    if pattern == "all":
        assert len(new_pix) == 0 and (depth <= 0).any()
    if pattern == "some" and n_old > 257:
        assert all(pix_of[r] >= 0 for r in (255, 256, 257))
    leaves = [dev(a).requires_grad_(True) for a in old + [cc] + frame + [alpha]]
    out = ops.FuseAppendFunction.apply(*leaves, dev(depth), dev(best), renorm)
    n1 = out[0].shape[0]
    assert n1 == n_old + len(new_pix)
    Wt = [bc.weights((n1, c), 30 + i) for i, c in enumerate((3, 3, 3, 1))]
    sum((o_ * dev(w)).sum() for o_, w in zip(out, Wt)).backward()
    merged = bool((pix_of >= 0).any())
    ob, cb, fbar, ab = fb.fuse_backward([a.astype(np.float64) for a in old], cc[:, 0].astype(np.float64),
                                        [a.reshape(P, 3).astype(np.float64) for a in frame],
                                        alpha.reshape(-1).astype(np.float64), pix_of, new_pix,
                                        [w.astype(np.float64) for w in Wt[:3]], Wt[3][:, 0].astype(np.float64),
                                        merged=merged, renorm_all=renorm)
    got = [host(t.grad) for t in leaves]
    got_old, got_cc = got[:3], got[3][:, 0]
    got_f, got_a = [g.reshape(P, 3) for g in got[4:7]], got[7].reshape(-1)
    tag = "fuse %dx%d n_old=%d %s renorm=%d" % (H, W, n_old, pattern, renorm)
    # copies and exact zeros
    identity = ~((pix_of >= 0) | (merged and renorm)) if n_old else np.zeros(0, bool)
    touched = np.zeros(P, bool)
    touched[new_pix] = True
    touched[pix_of[pix_of >= 0]] = True
    for t in range(3):
        assert np.array_equal(bits(got_old[t][identity]), bits(Wt[t][:n_old][identity])), "identity rows are copies"
        assert np.array_equal(bits(got_f[t][new_pix]), bits(Wt[t][n_old:])), "appended rows are copies"
        assert np.all(got_f[t][~touched] == 0)
        assert np.array_equal(got_old[t] != 0, ob[t] != 0) and np.array_equal(got_f[t] != 0, fbar[t] != 0)
    assert np.array_equal(bits(got_cc[identity]), bits(Wt[3][:n_old, 0][identity]))
    assert np.array_equal(bits(got_a[new_pix]), bits(Wt[3][n_old:, 0])) and np.all(got_a[~touched] == 0)
    assert np.array_equal(got_cc != 0, cb != 0) and np.array_equal(got_a != 0, ab != 0)
    # everything else
    for t in range(3):
        if n_old:
            within(tag + " old[%d]" % t, got_old[t], ob[t], FUSE_BAR)
        within(tag + " frame[%d]" % t, got_f[t], fbar[t], FUSE_BAR)
    if n_old:
        within(tag + " ccounts", got_cc, cb, FUSE_BAR)
    within(tag + " alpha", got_a, ab, FUSE_BAR)


# ------------------------------------------------------------------------------------------------ ICP backward
def read_tape(tape, ns, kw, init):
    """The forward tape of gs_icp_tape_f32 (gs_icp_tape_carve: trace, sys, src, idx, each 256-byte aligned) as the
    dictionary oracle/icp_backward.py differentiates."""
    K = int(kw.get("numiters", 20))
    raw = tape.cpu().numpy()
    Kc, n = max(K, 1), max(ns, 1)
    al = lambda x: (x + 255) // 256 * 256   # noqa: E731
    o = 0
    trace = raw[o:o + 48 * Kc].view(np.float32).reshape(Kc, 12)
    o += al(48 * Kc)
    sys_ = raw[o:o + 112 * Kc].view(np.float32).reshape(Kc, 28)
    o += al(112 * Kc)
    src = raw[o:o + 12 * Kc * n].view(np.float32).reshape(Kc, n, 3)
    o += al(12 * Kc * n)
    idx = raw[o:o + 8 * Kc * n].view(np.int32).reshape(Kc, 2, n)
    prm = dict(numiters=K, damp=1e-8, lambda_max=kw.get("lambda_max", 2.0), B=kw.get("B", 1.0), B2=kw.get("B2", 1.0),
               nu=kw.get("nu", 200.0), mode=kw.get("mode", 1))
    return dict(src=src[:K], idx=idx[:K], sys=sys_[:K], trace=trace[:K], init=np.asarray(init, np.float32), prm=prm)


def hip_icp(ops, src, tgt, tn, init, T_bar, need=(True, True, True, True), **kw):
    """(T, tape tensor, the four gradients as numpy or None)"""
    s, t, n, i = dev(src), dev(tgt), dev(tn), dev(init)
    T, _, tape, prm = ops.icp_with_tape(s, t, n, i, **kw)
    grads = ops.icp_backward(tape, prm, s, t, n, i, dev(T_bar), need)
    torch.cuda.synchronize()
    return host(T), tape, [None if g is None else host(g) for g in grads]


def check_icp(ops, tag, src, tgt, tn, init, T_bar, **kw):
    """HIP backward against the float64 oracle on the tape the HIP forward recorded; returns (T, tape dict, grads, oracle)"""
    T, tape, got = hip_icp(ops, src, tgt, tn, init, T_bar, **kw)
    tp = read_tape(tape, src.shape[0], kw, init)
    ref = ib.icp_backward(tp, tgt, tn, T_bar, src)
    for g, r, name in zip(got, ref, ("src", "tgt", "tn", "init")):
        assert g.shape == r.shape
        if np.all(r == 0):
            assert np.all(g == 0), (tag, name)
        else:
            within("%s %s_bar" % (tag, name), g, r, ICP_ORACLE_BAR)
    assert np.all(got[3][3] == 0)
    return T, tp, got, ref


def icp_init():
    from oracle.make_golden import icp_init_transform
    return icp_init_transform()


@pytest.fixture()
def det_mode():
    """switches GRADSLAM_HIP_DETERMINISTIC_BACKWARD inside the process (the library reads it on every call)"""
    old = os.environ.get("GRADSLAM_HIP_DETERMINISTIC_BACKWARD")

    def switch(on):
        os.environ["GRADSLAM_HIP_DETERMINISTIC_BACKWARD"] = "1" if on else "0"
    yield switch
    if old is None:
        os.environ.pop("GRADSLAM_HIP_DETERMINISTIC_BACKWARD", None)
    else:
        os.environ["GRADSLAM_HIP_DETERMINISTIC_BACKWARD"] = old


@pytest.mark.parametrize("mode,tag", [(1, "grad"), (0, "hard")])
def test_icp_backward_with_a_non_identity_init(ops, golden, det_mode, mode, tag):
    """gs_bwd_src_out_kernel rotates the source adjoint by `init`, and init_bar collects the source sums: both invisible
    at init = I.  Against the oracle and against the reference's own autograd (tests/golden/icp_init_grad.npz)."""
    g, u = golden("icp_init_grad"), golden("icp_unit")
    assert np.array_equal(g["init"], icp_init())
    for det in (False, True):
        det_mode(det)
        T, _, got, _ = check_icp(ops, "init!=I mode %d det %d" % (mode, det), u["src"], u["tgt"], u["tgt_normals"],
                                 g["init"], g["W"], numiters=5, mode=mode)
        np.testing.assert_allclose(T, g[tag + "_T"], atol=2e-5, rtol=0)
        for have, name in zip(got, ("src", "tgt", "tn", "init")):
            ref = g[tag + "_" + name]
            # (the reference also differentiates the constant bottom row of init; this project reports zero there)
            have, ref = (have[:3], ref[:3]) if name == "init" else (have, ref)
            within("init!=I mode %d det %d %s vs reference" % (mode, det, name), have, ref, ICP_REFERENCE_BAR)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("K", [0, 64])
def test_icp_backward_iteration_limits(ops, golden, K, mode):
    """numiters = 0 (T = init: its own branch) and 64 (the limit of the backward state)."""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    T, _, got, _ = check_icp(ops, "K=%d mode %d" % (K, mode), u["src"], u["tgt"], u["tgt_normals"], icp_init(), W,
                             numiters=K, mode=mode)
    if K == 0:
        assert np.array_equal(T, icp_init()) and np.all(got[0] == 0) and np.all(got[1] == 0) and np.all(got[2] == 0)
        assert np.array_equal(bits(got[3][:3]), bits(W[:3]))


def test_icp_backward_refuses_65_iterations(ops, golden):
    """the backward state holds 64 iterations: 65 is an error, not a result"""
    from gradslam_amd._C import HipExtensionError
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    s, t, n, i = dev(u["src"]), dev(u["tgt"]), dev(u["tgt_normals"]), dev(np.eye(4, dtype=np.float32))
    T, _, tape, prm = ops.icp_with_tape(s, t, n, i, numiters=65)
    assert torch.isfinite(T).all()
    with pytest.raises(HipExtensionError, match="numiters"):
        ops.icp_backward(tape, prm, s, t, n, i, dev(W))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n_src", [1, 255, 257])
def test_icp_backward_source_counts_around_a_block(ops, golden, n_src, mode):
    """one source point, one short of a block and one past it, against the ~700 targets of icp_unit"""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    src = np.ascontiguousarray(u["src"][:: max(u["src"].shape[0] // n_src, 1)][:n_src])
    assert src.shape[0] == n_src and u["tgt"].shape[0] > 600
    check_icp(ops, "n_src=%d mode %d" % (n_src, mode), src, u["tgt"], u["tgt_normals"], icp_init(), W, numiters=5,
              mode=mode)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("mode", [1, 0])
def test_icp_backward_single_target_shared_by_every_source(ops, golden, det_mode, mode, det):
    """every source point adds into the same target: the worst case for the float64 atomics, and one run of n_src pairs
    for the deterministic mode's segmented sum"""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    det_mode(det)
    j = u["tgt"].shape[0] // 2
    _, tp, _, _ = check_icp(ops, "one target mode %d det %d" % (mode, det), u["src"], u["tgt"][j:j + 1],
                            u["tgt_normals"][j:j + 1], icp_init(), W, numiters=5, mode=mode)
    assert np.all(tp["idx"] == 0)


@pytest.mark.parametrize("mode", [1, 0])
def test_icp_backward_deterministic_mode_against_the_oracle(ops, golden, det_mode, mode):
    """GRADSLAM_HIP_DETERMINISTIC_BACKWARD=1 on the icp_unit case at the bar of the atomic mode, not merely close to it"""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    det_mode(True)
    _, _, a, _ = check_icp(ops, "det mode %d" % mode, u["src"], u["tgt"], u["tgt_normals"], icp_init(), W, numiters=20,
                           mode=mode)
    _, _, b, _ = check_icp(ops, "det mode %d again" % mode, u["src"], u["tgt"], u["tgt_normals"], icp_init(), W,
                           numiters=20, mode=mode)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)), "the deterministic mode gives the same bits twice"


@pytest.mark.parametrize("mode", [1, 0])
def test_icp_backward_threshold_that_rejects_every_pair(ops, golden, mode):
    """no pair survives dist_thresh: the point gradients are exactly zero, init_bar is what the oracle says"""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    _, tp, got, ref = check_icp(ops, "all rejected mode %d" % mode, u["src"], u["tgt"], u["tgt_normals"], icp_init(), W,
                                numiters=5, mode=mode, dist_thresh=1e-12)
    assert np.all(tp["idx"] < 0)
    assert all(np.all(g == 0) for g in got[:3]) and all(np.all(r == 0) for r in ref[:3])
    assert np.abs(ref[3]).max() > 0


@pytest.mark.parametrize("det", [False, True])
def test_icp_backward_single_leaf_subsets(ops, golden, det_mode, det):
    """a NULL output pointer must not change the other outputs: each single-leaf run equals its entry of the all-leaves
    run.  The source and init adjoints never pass through an atomic, nor does anything in the deterministic mode: equal
    bits; the target adjoints of the atomic mode may differ by the order of float64 additions (1e-16) before the one
    rounding to float32, i.e. by at most one float32 ulp of an element."""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    det_mode(det)
    args = (u["src"], u["tgt"], u["tgt_normals"], icp_init(), W)
    _, _, full = hip_icp(ops, *args, numiters=5)
    for leaf in range(4):
        need = tuple(i == leaf for i in range(4))
        _, _, one = hip_icp(ops, *args, need=need, numiters=5)
        assert all((g is None) == (not nd) for g, nd in zip(one, need))
        if det or leaf in (0, 3):
            assert np.array_equal(bits(one[leaf]), bits(full[leaf])), leaf
        else:
            assert np.all(np.abs(one[leaf] - full[leaf]) <= np.spacing(np.abs(full[leaf]))), leaf


@pytest.mark.parametrize("mode", [1, 0])
def test_icp_backward_non_default_lm_parameters(ops, golden, mode):
    """two iterations, before the solve has converged: there the float64 oracle's gradients move by 3 to 9 % between
    the default and these parameters (after five they agree to 1e-6: the fixed point does not depend on the schedule)"""
    u, W = golden("icp_unit"), golden("icp_grad")["W"]
    kw = dict(numiters=2, mode=mode, lambda_max=3.0, B=0.7, B2=1.3, nu=50.0)
    T0, _, base = hip_icp(ops, u["src"], u["tgt"], u["tgt_normals"], icp_init(), W, numiters=2, mode=mode)
    T, _, got, _ = check_icp(ops, "LM parameters mode %d" % mode, u["src"], u["tgt"], u["tgt_normals"], icp_init(), W, **kw)
    if mode == 1:   # the soft schedule uses all four; they must have changed the problem
        assert not np.array_equal(T, T0) and bc.rel_err(got[0], base[0]) > 1e-2
