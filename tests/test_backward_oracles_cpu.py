"""The float64 numpy adjoints that tests/test_hip_backward_kernels.py points at the HIP backward kernels, each pinned
here on the CPU: against central finite differences of its own float64 forward, and (ICP with a non-identity initial
transform) against the reference's autograd (tests/golden/icp_init_grad.npz, oracle/make_golden.py --icp-init).
Also recomputes the float32-against-float64 gaps that bound the float32 kernels (tests/backward_cases.py)."""
import numpy as np
import pytest

from oracle import fusion_backward as fb
from oracle import icp_backward as ib
from oracle import maps_backward as mb

from . import backward_cases as bc


def fd_check(loss, x, ana, picks, h=1e-6, tol=1e-6):
    """central differences of loss(x) at the picked indices of x against the analytic adjoint"""
    for idx in picks:
        e = np.zeros_like(x)
        e[idx] = h
        num = (loss(x + e) - loss(x - e)) / (2 * h)
        assert abs(num - ana[idx]) <= tol * max(1.0, abs(num)), (idx, num, ana[idx])


# ------------------------------------------------------------------------------------------------ frame maps
def _smooth_depth(H, W, rng, base):
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return base + 0.1 * np.sin(0.9 * h + 0.3) * np.cos(0.7 * w) + 0.05 * rng.random((H, W))


@pytest.mark.parametrize("H,W", [(2, 2), (2, 7), (7, 2), (5, 6)])
@pytest.mark.parametrize("fy", [1.0, -1.0])
def test_frame_maps_adjoint_by_finite_differences(H, W, fy):
    """depth_bar and K_bar of oracle/maps_backward.py at H = 2 / W = 2 (both border terms fall on the same pixel), with a
    hole, a negative depth and a frame that straddles the alpha clamp (|v| from 3.1 to 3.7 m at sigma 0.6)."""
    rng = np.random.default_rng(H * 100 + W)
    K = np.eye(4)
    # focal lengths that are exact in float32, so that the float32 inverse intrinsics of the adjoint are the float64 ones
    # of the finite-difference forward up to 1e-8
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 8.0, 8.0 * fy, 0.5 * W, 0.5 * H
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.sqrt(((w - K[0, 2]) / K[0, 0]) ** 2 + ((h - K[1, 2]) / K[1, 1]) ** 2 + 1.0)
    depth = _smooth_depth(H, W, rng, np.where((h + w) % 2 == 0, 3.1, 3.7)) / ray
    depth.reshape(-1)[:: max(H * W // 2, 3)][1:] = 0.0
    if H * W > 4:
        depth[-1, -1] = -1.0
    Wv, Wn, Wa = rng.standard_normal((H, W, 3)), rng.standard_normal((H, W, 3)), 1e4 * rng.standard_normal((H, W))
    _, _, a = mb.frame_maps_forward(depth, K, bc.SIGMA)
    valid = depth > 0
    assert (a[valid] > 1e-7).any() and (a[valid] == 1e-7).any(), "the frame must straddle the clamp"

    def loss_d(d):
        V, N, al = mb.frame_maps_forward(d, K, bc.SIGMA)
        return (V * Wv).sum() + (N * Wn).sum() + (al * Wa).sum()

    def loss_K(Km):
        Kp = K.copy()
        Kp[:2, :3] = Km
        V, N, al = mb.frame_maps_forward(depth, Kp, bc.SIGMA)
        return (V * Wv).sum() + (N * Wn).sum() + (al * Wa).sum()

    d_bar, K_bar = mb.frame_maps_backward(depth, K, bc.SIGMA, Wv, Wn, Wa, want_K=True)
    assert np.all(d_bar[~valid] == 0)
    fd_check(loss_d, depth, d_bar, [tuple(i) for i in np.argwhere(valid)], tol=2e-5)
    assert np.count_nonzero(K_bar) == 4 and np.all(K_bar[3] == 0)
    # (fx + 1e-6 in the adjoint, fx in the forward: 1e-7 relative)
    fd_check(loss_K, K[:2, :3].copy(), K_bar[:2, :3], [(0, 0), (0, 2), (1, 1), (1, 2)], tol=2e-5)


# ------------------------------------------------------------------------------------------------ global maps
@pytest.mark.parametrize("use", ["gv", "gn", "gvgn"])
def test_global_maps_adjoint_by_finite_differences(use):
    rng = np.random.default_rng(3)
    H, W = 4, 5
    v, n = rng.standard_normal((H, W, 3)), rng.standard_normal((H, W, 3))
    depth = rng.random((H, W)) - 0.3
    pose = ib.se3_exp(np.array([0.4, -0.3, 0.2, 0.5, -0.7, 0.3]))
    Wg = rng.standard_normal((H, W, 3)) if "gv" in use else None
    Wn = rng.standard_normal((H, W, 3)) if "gn" in use else None

    def loss(v_, n_, pose_):
        gv, gn = mb.global_maps_forward(v_, n_, depth, pose_)
        return (0.0 if Wg is None else (gv * Wg).sum()) + (0.0 if Wn is None else (gn * Wn).sum())

    vb, nb, pb = mb.global_maps_backward(v, n, depth, pose, Wg, Wn)
    assert (vb is None) == (Wg is None) and (nb is None) == (Wn is None) and np.all(pb[3] == 0)
    every = [tuple(i) for i in np.argwhere(np.ones((H, W, 3), bool))]
    if vb is not None:
        assert np.all(vb[depth <= 0] == 0)
        fd_check(lambda x: loss(x, n, pose), v, vb, every)
    if nb is not None:
        fd_check(lambda x: loss(v, x, pose), n, nb, every)
    fd_check(lambda x: loss(v, n, x), pose, pb, [(i, j) for i in range(3) for j in range(4)])


# ------------------------------------------------------------------------------------------------ down-sampler
@pytest.mark.parametrize("ds", [1, 2, 4, 5])
def test_downsample_adjoint_is_the_transpose_of_the_gather(ds):
    rng = np.random.default_rng(ds)
    H, W = 7, 11
    depth = rng.random((H, W)) - 0.25
    g = rng.standard_normal((H, W, 3))
    pts = mb.downsample_forward(g, depth, ds)
    lat = np.zeros((H, W), bool)
    lat[::ds, ::ds] = True
    assert pts.shape[0] == int((lat & (depth > 0)).sum()) and np.array_equal(pts, g[lat & (depth > 0)])
    pb = rng.standard_normal(pts.shape)
    gb = mb.downsample_backward(pb, depth, ds)
    assert np.array_equal(gb[lat & (depth > 0)], pb) and np.all(gb[~(lat & (depth > 0))] == 0)
    assert abs((pts * pb).sum() - (g * gb).sum()) < 1e-12      # <G x, y> = <x, G^T y>


# ------------------------------------------------------------------------------------------------ alpha
def test_alpha_adjoint_by_finite_differences():
    rng = np.random.default_rng(9)
    p = bc.alpha_points(40).astype(np.float64)
    Wa = 1e4 * rng.standard_normal(40)
    two = float(np.float32(2 * bc.SIGMA ** 2))
    a = np.exp(-(p * p).sum(1) / two)
    assert (a > 1e-7).any() and (a < 1e-7).any()

    def loss(p_, sigma_scale=1.0):
        return (np.clip(np.exp(-(p_ * p_).sum(1) / (two * sigma_scale ** 2)), np.float32(1e-7), np.float32(1.01)) * Wa).sum()

    pb, sb = mb.alpha_backward(p, bc.SIGMA, 1e-7, Wa)
    assert np.all(pb[a < 1e-7] == 0)
    fd_check(lambda x: loss(x), p, pb, [(i, c) for i in range(40) for c in range(3)], h=1e-5, tol=1e-5)
    h = 1e-5
    num = (loss(p, 1 + h) - loss(p, 1 - h)) / (2 * h) / bc.SIGMA        # d / d sigma = (1 / sigma) d / d scale
    assert abs(num - sb) <= 1e-5 * abs(num)


# ------------------------------------------------------------------------------------------------ fuse
def _fuse_case(n, P, matched, rng, zero_row=True):
    old = [rng.standard_normal((n, 3)) for _ in range(3)]
    cc = rng.random(n) + 0.1
    frame = [rng.standard_normal((P, 3)) for _ in range(3)]
    alpha = rng.random(P)
    pix_of = np.full(n, -1)
    rows = rng.choice(n, matched, replace=False) if matched else np.zeros(0, int)
    pixs = rng.choice(P, matched, replace=False)
    pix_of[rows] = pixs
    if zero_row and matched:           # cc + alpha == 0: a zero-confidence row merged with a zero-alpha pixel
        cc[rows[0]], alpha[pixs[0]] = 0.0, 0.0
    if zero_row and matched > 1:       # and with a non-zero numerator cc x + alpha f: cc = -alpha
        cc[rows[1]] = -alpha[pixs[1]]
    if (pix_of < 0).any():
        cc[np.flatnonzero(pix_of < 0)[0]] = 0.0   # an unmatched zero-confidence row
    free = np.setdiff1d(np.arange(P), pixs)
    new_pix = np.sort(rng.choice(free, max(len(free) // 2, 0), replace=False)) if len(free) else np.zeros(0, int)
    return old, cc, frame, alpha, pix_of, new_pix


@pytest.mark.parametrize("renorm_all", [True, False])
@pytest.mark.parametrize("n,P,matched", [(12, 20, 5), (12, 20, 0), (0, 9, 0), (1, 9, 1), (6, 6, 6)])
def test_fuse_adjoint_by_finite_differences_all_modes(n, P, matched, renorm_all):
    """renorm_all False and True, a `cc + alpha == 0` row, n_old = 0, no match anywhere (identity), every pixel matched
    (no appended row)."""
    rng = np.random.default_rng(n * 100 + P + matched)
    old, cc, frame, alpha, pix_of, new_pix = _fuse_case(n, P, matched, rng)
    merged = matched > 0
    nk = n + len(new_pix)
    Wt = [rng.standard_normal((nk, 3)) for _ in range(3)]
    Wc = rng.standard_normal(nk)

    def loss(old_, cc_, frame_, alpha_):
        out, c2 = fb.fuse_forward(old_, cc_, frame_, alpha_, pix_of, new_pix, merged, renorm_all)
        return sum((o_ * w).sum() for o_, w in zip(out, Wt)) + (c2 * Wc).sum()

    ob, cb, fbar, ab = fb.fuse_backward(old, cc, frame, alpha, pix_of, new_pix, Wt, Wc, merged, renorm_all)
    rewritten = (pix_of >= 0) | (merged and renorm_all)
    for t in range(3):
        assert np.array_equal(ob[t][~rewritten], Wt[t][:n][~rewritten])          # identity rows: copies
        assert np.array_equal(fbar[t][new_pix], Wt[t][n:])                      # appended rows: copies
        fd_check(lambda x: loss([x if k == t else old[k] for k in range(3)], cc, frame, alpha), old[t], ob[t],
                 [(i, c) for i in range(n) for c in range(3)])
        fd_check(lambda x: loss(old, cc, [x if k == t else frame[k] for k in range(3)], alpha), frame[t], fbar[t],
                 [(i, c) for i in range(P) for c in range(3)])
    assert np.array_equal(cb[~rewritten], Wc[:n][~rewritten]) and np.array_equal(ab[new_pix], Wc[n:])
    touched = np.zeros(P, bool)
    touched[new_pix] = True
    touched[pix_of[pix_of >= 0]] = True
    assert np.all(ab[~touched] == 0) and all(np.all(f[~touched] == 0) for f in fbar)
    # rows whose cc' = cc + alpha is zero sit on the `where(cc' == 0, 1, cc')` kink: the guard gives them a zero
    # derivative through 1 / cc' and a difference quotient is not defined there
    a_of = np.where(pix_of >= 0, alpha[np.maximum(pix_of, 0)], 0.0)
    kink = rewritten & (cc + a_of == 0)
    assert not merged or kink.any()
    fd_check(lambda x: loss(old, x, frame, alpha), cc, cb, [i for i in range(n) if not kink[i]])
    kink_pix = set(pix_of[kink & (pix_of >= 0)].tolist())
    fd_check(lambda x: loss(old, cc, frame, x), alpha, ab, [p for p in range(P) if p not in kink_pix])
    # on the kink itself 1 / cc' is the constant 1: x' = cc x + a f, and cc' = cc + a feeds the new confidence only
    for i in np.flatnonzero(kink):
        xb = sum((Wt[t][i] * old[t][i]).sum() for t in range(3))
        assert cb[i] == pytest.approx(Wc[i] + xb, abs=1e-12)


# ------------------------------------------------------------------------------------------------ ICP, init != I
@pytest.mark.parametrize("tag,mode", [("grad", 1), ("hard", 0)])
def test_numpy_icp_backward_oracle_with_initial_transform_matches_reference_autograd(golden, tag, mode):
    """gradICP and hard-LM ICP, 5 iterations, started from a transform a few centimetres / one degree off the identity:
    the three point gradients AND the gradient of `init` against the reference's own autograd, at the bars of
    test_numpy_backward_oracle_matches_reference_autograd.  (The reference also reports a gradient for the constant
    bottom row of `init`; this project's convention is zero there, and the top three rows are compared.)"""
    g, u = golden("icp_init_grad"), golden("icp_unit")
    assert np.abs(g["init"] - np.eye(4)).max() > 1e-2
    T, tape = ib.icp_forward_tape(u["src"], u["tgt"], u["tgt_normals"], init=g["init"], numiters=5, mode=mode)
    np.testing.assert_allclose(T, g[tag + "_T"], atol=2e-5, rtol=0)
    sb, tb, nb, ibar = ib.icp_backward(tape, u["tgt"], u["tgt_normals"], g["W"], u["src"])
    for have, name in ((sb, "src"), (tb, "tgt"), (nb, "tn"), (ibar[:3], "init")):
        ref = g[tag + "_" + name][:3] if name == "init" else g[tag + "_" + name]
        assert bc.rel_err(have, ref) < 5e-4, name
    assert np.all(ibar[3] == 0)


# ------------------------------------------------------------------------------------------------ float32 yardsticks
def _same_gap(now, const):
    """a recomputed gap against its constant: within DRIFT either way; gaps so small that the 8-ulp floor is the bound
    anyway only have to stay that small"""
    irrelevant = bc.FLOOR_ULPS * bc.EPS32 / bc.KERNEL_FACTOR
    if const <= irrelevant:
        return now <= irrelevant
    return const / bc.DRIFT <= now <= const * bc.DRIFT


@pytest.mark.parametrize("H,W", bc.FRAME_SIZES)
def test_frame_gap_constants_are_current(H, W):
    for fy, scale in bc.FRAME_VARIANTS:
        depth, K = bc.frame_case(H, W, fy, scale)
        V, _, a = mb.frame_maps_forward(depth, K, bc.SIGMA)
        valid = depth > 0
        assert valid.any()
        if H > 2 and W > 2:
            assert (depth < 0).any() and valid[H - 1].any() and valid[:, W - 1].any() and not valid[0, W - 1]
        if scale == "clamp":
            assert (a[valid] > 1e-7).any() and (a[valid] == 1e-7).any(), "valid pixels on both sides of the clamp"
        for loss in bc.FRAME_LOSSES:
            key = bc.frame_key(H, W, fy, scale, loss)
            now, const = bc.frame_gaps(H, W, fy, scale, loss), bc.FRAME_GAP[key]
            assert _same_gap(now[0], const[0]) and _same_gap(now[1], const[1]), (key, now, const)


@pytest.mark.parametrize("H,W", bc.FRAME_SIZES)
def test_global_gap_constants_are_current(H, W):
    for loss in bc.GLOBAL_LOSSES:
        key = "%dx%d/%s" % (H, W, loss)
        now, const = bc.global_gaps(H, W, loss), bc.GLOBAL_GAP[key]
        assert all((a is None) == (b is None) and (a is None or _same_gap(a, b)) for a, b in zip(now, const)), (key, now, const)


def test_alpha_gap_constants_are_current():
    for n in bc.ALPHA_SIZES:
        now, const = bc.alpha_gaps(n), bc.ALPHA_GAP[n]
        assert _same_gap(now[0], const[0]) and _same_gap(now[1], const[1]), (n, now, const)


@pytest.mark.parametrize("renorm_all", [True, False])
def test_fuse_forward_restatement_matches_the_reference_pinned_oracle(renorm_all):
    """oracle/fusion_backward.fuse_forward (what the finite differences above differentiate) against oracle.fuse_append,
    the C restatement pinned to the reference's fuse_with_map, for renorm_all False and True."""
    from oracle import oracle as o
    rng = np.random.default_rng(4)
    H, W, n = 5, 7, 40
    old, cc, frame, alpha, pix_of, _ = _fuse_case(n, H * W, 12, rng)
    depth = rng.random((H, W)) + 0.5
    unmatched = np.setdiff1d(np.arange(H * W), pix_of[pix_of >= 0])
    depth.reshape(-1)[unmatched[::3]] = 0.0
    best = np.full(H * W, -1, np.int32)
    best[pix_of[pix_of >= 0]] = np.flatnonzero(pix_of >= 0)
    new_pix = np.flatnonzero((depth.reshape(-1) > 0) & (best < 0))
    f32 = [a.astype(np.float32) for a in old + [cc[:, None]] + frame + [alpha]]
    P, N, C, F = o.fuse_append(f32[0], f32[1], f32[2], f32[3], best, f32[4].reshape(H, W, 3), f32[5].reshape(H, W, 3),
                               f32[6].reshape(H, W, 3), f32[7].reshape(H, W), depth.astype(np.float32),
                               renorm_all=renorm_all)
    out, c2 = fb.fuse_forward([a.astype(np.float64) for a in f32[:3]], f32[3][:, 0].astype(np.float64),
                              [a.astype(np.float64) for a in f32[4:7]], f32[7].astype(np.float64), pix_of, new_pix,
                              True, renorm_all)
    for have, want in zip((P, N, C, F[:, 0]), out + [c2]):
        assert have.shape == want.shape and np.abs(have - want).max() < 1e-5
    untouched = np.flatnonzero(pix_of < 0)
    if not renorm_all:
        assert np.array_equal(P[untouched], f32[0][untouched]) and np.array_equal(F[untouched], f32[3][untouched])
