"""The scalar stage of every ICP driver -- hard-LM accept / reject, gradLM soft update, se3_exp, the 4x4 accumulation
into the pose -- against the float64 restatement of tests/icp_lm_ref.py, on the scenes of tests/icp_lm_cases.py.

Three engines run every case in both modes: the brute-force driver (ops.icp at 96 points: the scalar copy of the stage),
the half-iteration driver (ops.icp at 640 points with device-side counts: the one-wave copy on LDS) and the tape entry
point (ops.icp_with_tape at 96 points; its trace is the first K x 12 floats of the tape).  Everything runs in this
process: no environment switches, no child processes.

Bounds (none is tuned against a kernel; every figure is printed before it is asserted):
  mode 0   damp and sig on the bits (halving and doubling are exact); T as below.
  mode 1   sig: 4 float32 roundings lie between errdiff and sig (the exponential, 1 + e, the power, the reciprocal), each
           of which may fall the other way when gs_exp_fast / gs_log_fast differ from libm in the last bit of the double,
           and none of the four operations amplifies a relative difference (the power damps it by 1 / nu): 4 eps32
           relative, eps32 = 2^-23.  The damping factor has 4 (the exponential, 1 + e, the quotient, lmin + q; both terms
           are positive) and the product with the previous damping 1 more; replay carries its own damping from the
           initial one, so after iteration k the bound is 5 (k + 1) eps32.
  T        a polynomial good to an ulp of double, once rounded, moves an entry of se3_exp by at most one float32 ulp:
           |dS| <= eps32 |S| entry by entry.  In mode 1 the step is se3_exp(sig * xi) and sig may differ by 4 eps32 (5
           with the product's rounding): the rotation block moves by at most 5 eps32 theta, the translation by at most
           5 eps32 |v| (1 + theta)^2.  Through T_k = S_k T_(k-1): E_k <= dS_k |T_(k-1)| + |S_k| E_(k-1), plus 4 eps32
           |S_k| |T_(k-1)| for the roundings of a float32 product of slightly different factors (4 products, 3 sums per
           entry); the bottom row is exact.  pose_bound() computes E_K from replay's own matrices.
Measured on an MI355X (arithmetic contract): 0 ulps for damp, sig and every entry of T, everywhere.
Against the oracle, on the cases that are decisive (every |new_err - err| >= 1e-3 err on the oracle's trace): the same
accept / reject pattern, mode 0 damp on the bits, mode 1 factor and sig inside [f(d - delta), f(d + delta)] of the
float64 formula at the oracle's errdiff d, delta = 1e-4 (err + new_err), widened by the bounds above, and T within the
1e-6 of test_icp_against_oracle_and_reference."""
import functools

import numpy as np
import pytest
import torch

from oracle import icp_backward as ib
from oracle import oracle as o
from tests import backward_cases as bc
from tests import icp_lm_cases as lc
from tests import icp_lm_ref as lm

pytestmark = pytest.mark.gpu

EPS32 = lm.EPS32
SIG_ROUNDINGS, FACTOR_ROUNDINGS = 4, 5
CASE_IDS = [c["name"] for c in lc.CASES]
ENGINES = ("brute96", "grid640", "tape96")
ENGINE_N = {"brute96": lc.N_BRUTE, "grid640": lc.N_GRID, "tape96": lc.N_BRUTE}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()   # (a copy: the shared scenes are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _count(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


_RUNS = {}


def run(ops, case, engine, mode):
    """(T, trace) of one engine on one case, computed once and shared (read-only)"""
    key = (case["name"], engine, mode)
    if key not in _RUNS:
        n = ENGINE_N[engine]
        src, tgt, tn = (dev(a) for a in lc.clouds(case, n))
        kw = lc.icp_kwargs(case, n, mode)
        K = kw["numiters"]
        if engine == "tape96":
            T, _, tape, _ = ops.icp_with_tape(src, tgt, tn, **kw)
            tr = tape[: 4 * 12 * K].view(torch.float32).view(K, 12)
        elif engine == "grid640":
            T, tr = ops.icp(src, tgt, tn, return_idx=False, return_trace=True, n_src_dev=_count(n), n_tgt_dev=_count(n),
                            **kw)
        else:
            T, tr = ops.icp(src, tgt, tn, return_idx=False, return_trace=True, **kw)
        T, tr = host(T).copy(), host(tr).copy()
        T.setflags(write=False)
        tr.setflags(write=False)
        _RUNS[key] = (T, tr)
    return _RUNS[key]


def pose_bound(r, trace, prm):
    """entrywise bound on |T_kernel - T_replay| (module docstring), from replay's own matrices"""
    E = np.zeros((4, 4))
    T = np.eye(4)
    for k in range(trace.shape[0]):
        if not r["accept"][k]:
            continue
        S = r["T_step"][k].astype(np.float64)
        dS = EPS32 * np.abs(S)
        if prm["mode"] == 1:
            xs = (r["sig"][k] * trace[k, 4:10]).astype(np.float32)
            th, v = lm.theta_of(xs), float(np.linalg.norm(xs[:3].astype(np.float64)))
            dS[:3, :3] += (SIG_ROUNDINGS + 1) * EPS32 * th
            dS[:3, 3] += (SIG_ROUNDINGS + 1) * EPS32 * v * (1.0 + th) ** 2
        prod = np.abs(S) @ np.abs(T)
        E = dS @ np.abs(T) + np.abs(S) @ E + (4 * EPS32 * prod if (E.any() or dS.any()) else 0.0)
        E[3] = 0.0
        T = S @ T
    return E


def rel_eps(got, ref):
    """|got - ref| / |ref| in units of eps32, per element (0 where both are equal, zeros and infinities included)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref) / np.abs(ref) / EPS32
    return np.where(got == ref, 0.0, np.where(np.isfinite(d), d, np.inf))


# ------------------------------------------------------------------------------------------------ self-consistency
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_kernel_trace_replays_to_its_own_damp_sig_and_pose(ops, case, engine, mode):
    """From the kernel's own err, new_err and xi the restatement must reproduce the kernel's damp, sig and final T."""
    n = ENGINE_N[engine]
    prm = lc.params(case, n, mode)
    T, tr = run(ops, case, engine, mode)
    assert np.isfinite(T).all() and np.isfinite(tr).all()
    assert np.array_equal(tr[:, 10:], np.zeros((tr.shape[0], 2), np.float32))
    r = lm.replay(tr, prm)
    tag = "%s/%s/mode%d" % (case["name"], engine, mode)
    if mode == 0:
        assert np.array_equal(bits(tr[:, 2]), bits(r["damp"])), (tag, tr[:, 2], r["damp"])
        assert np.array_equal(bits(tr[:, 3]), bits(np.ones(tr.shape[0], np.float32))), (tag, tr[:, 3])
    else:
        k = np.arange(tr.shape[0])
        d_damp, d_sig = rel_eps(tr[:, 2], r["damp"]), rel_eps(tr[:, 3], r["sig"])
        print("%-28s damp %.2f eps32 (bound %d (k + 1))  sig %.2f eps32 (bound %d)  worst ulps: damp %.1f sig %.1f"
              % (tag, d_damp.max(), FACTOR_ROUNDINGS, d_sig.max(), SIG_ROUNDINGS,
                 lm.ulp_distance(tr[:, 2], r["damp"]).max(), lm.ulp_distance(tr[:, 3], r["sig"]).max()))
        assert np.all(d_damp <= FACTOR_ROUNDINGS * (k + 1)), (tag, d_damp)
        assert np.all(d_sig <= SIG_ROUNDINGS), (tag, d_sig)
    E = pose_bound(r, tr, prm)
    diff = np.abs(T.astype(np.float64) - r["T"].astype(np.float64))
    print("%-28s T: worst |dT| %.3e (%.1f ulps), bound there %.3e, pattern %s"
          % (tag, diff.max(), lm.ulp_distance(T, r["T"]).max(), E.flat[diff.argmax()], lc.pattern(tr)))
    assert np.all(diff <= E), (tag, diff, E)
    if mode == 0 and not E.any():   # (no accepted step at all: the initial pose, untouched)
        assert np.array_equal(T, np.eye(4, dtype=np.float32))
    if mode in case["witness_modes"]:
        assert case["witness"](tr, prm), (tag, lc.pattern(tr), tr[:, :4])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_a_rejected_iteration_leaves_the_pose_untouched(ops, case, engine):
    """mode 0: T after K iterations == T after the last accepted one (the solve cut there), on the bits -- the rejects
    behind it multiply nothing into T_total -- and every reject doubles the damping exactly."""
    n = ENGINE_N[engine]
    T, tr = run(ops, case, engine, 0)
    acc = tr[:, 1] < tr[:, 0]
    if case["witness"] in (lc.w_decisive0, lc.w_reaccept):
        assert acc.any() and not acc.all(), "these two cases mix accepts and rejects"
    if not acc.any():
        assert np.array_equal(T, np.eye(4, dtype=np.float32))
        return
    last = int(np.flatnonzero(acc)[-1]) + 1
    src, tgt, tn = (dev(a) for a in lc.clouds(case, n))
    kw = dict(lc.icp_kwargs(case, n, 0), numiters=last)
    if engine == "tape96":
        T_cut = ops.icp_with_tape(src, tgt, tn, **kw)[0]
    elif engine == "grid640":
        T_cut = ops.icp(src, tgt, tn, return_idx=False, n_src_dev=_count(n), n_tgt_dev=_count(n), **kw)
    else:
        T_cut = ops.icp(src, tgt, tn, return_idx=False, **kw)
    assert np.array_equal(bits(host(T_cut)), bits(T)), (case["name"], engine, lc.pattern(tr))
    prev = np.concatenate([[np.float32(lc.params(case, n, 0)["damp"])], tr[:-1, 2]]).astype(np.float32)
    assert np.array_equal(bits(tr[~acc, 2]), bits(prev[~acc] * np.float32(2)))
    assert np.array_equal(bits(tr[acc, 2]), bits(prev[acc] / np.float32(2)))


# ------------------------------------------------------------------------------------------------ against the oracle
def _decisive(engine):
    return [(c, m) for c in lc.CASES for m in c["decisive"][ENGINE_N[engine]]]


@pytest.mark.parametrize("engine", ENGINES)
def test_decisive_cases_follow_the_oracle(ops, engine):
    n = ENGINE_N[engine]
    pairs = _decisive(engine)
    assert len(pairs) >= 6
    for case, mode in pairs:
        prm = lc.params(case, n, mode)
        T, tr = run(ops, case, engine, mode)
        oT, otr = lc.oracle_run(case, n, mode)
        tag = "%s/%s/mode%d" % (case["name"], engine, mode)
        # the premise of the interval below: err and new_err within the rtol of test_icp_against_oracle_and_reference
        np.testing.assert_allclose(tr[:, :2], otr[:, :2], rtol=1e-4, atol=1e-9, err_msg=tag)
        assert lc.pattern(tr) == lc.pattern(otr), (tag, lc.pattern(tr), lc.pattern(otr))
        if mode == 0:
            assert np.array_equal(bits(tr[:, 2]), bits(otr[:, 2])), (tag, tr[:, 2], otr[:, 2])
        else:
            prev = np.concatenate([[float(np.float32(prm["damp"]))], tr[:-1, 2].astype(np.float64)])
            factor, sig = tr[:, 2].astype(np.float64) / prev, tr[:, 3].astype(np.float64)
            wf, ws = (FACTOR_ROUNDINGS + 1) * EPS32, SIG_ROUNDINGS * EPS32
            for k in range(tr.shape[0]):
                err, new_err = float(otr[k, 0]), float(otr[k, 1])
                d, delta = new_err - err, 1e-4 * (err + new_err)
                lo = lm.soft_formulas_f64(min(max(d - delta, -70.0), 70.0), prm)
                hi = lm.soft_formulas_f64(min(max(d + delta, -70.0), 70.0), prm)
                assert lo[0] * (1 - wf) <= factor[k] <= hi[0] * (1 + wf), (tag, k, factor[k], lo[0], hi[0])
                assert lo[1] * (1 - ws) <= sig[k] <= hi[1] * (1 + ws), (tag, k, sig[k], lo[1], hi[1])
        print("%-28s |T - oracle| %.3e  pattern %s" % (tag, np.abs(T - oT).max(), lc.pattern(tr)))
        np.testing.assert_allclose(T, oT, rtol=0, atol=1e-6, err_msg=tag)


# ------------------------------------------------------------------------------------------------ engine agreement
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["decisive0", "soft_mid"])
def test_brute_force_and_grid_drivers_agree_bit_for_bit(ops, name, mode):
    """One 640-point scene through the brute-force driver (no device counts: fewer than 2048 targets) and the grid driver
    (device counts).  The two searches return the same neighbours, so a difference is between the scalar copy of the
    stage and the one-wave copy."""
    case = lc.BY_NAME[name]
    n = lc.N_GRID
    src, tgt, tn = (dev(a) for a in lc.clouds(case, n))
    kw = lc.icp_kwargs(case, n, mode)
    Tb, ib_, trb = ops.icp(src, tgt, tn, return_trace=True, **kw)
    Tg, ig, trg = ops.icp(src, tgt, tn, return_trace=True, n_src_dev=_count(n), n_tgt_dev=_count(n), **kw)
    assert torch.equal(ib_, ig)
    assert np.array_equal(bits(host(trb)), bits(host(trg))), (host(trb), host(trg))
    assert np.array_equal(bits(host(Tb)), bits(host(Tg))), (host(Tb), host(Tg))
    _, tr = run(ops, case, "grid640", mode)
    assert np.array_equal(bits(host(trg)), bits(tr))


# ------------------------------------------------------------------------------------------------ se3_exp alone
def _f32_neighbours(x):
    x = np.float32(x)
    return [float(np.nextafter(x, np.float32(-np.inf))), float(x), float(np.nextafter(x, np.float32(np.inf)))]


THETAS = ([0.0, 1e-30] + _f32_neighbours(1e-6) + [1e-4] + _f32_neighbours(1.0) + _f32_neighbours(np.pi)
          + [2 * np.pi + 0.1, 50.0])
AXES = [np.array([1.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0), np.array([0.36, -0.48, 0.8])]
TRANSLATIONS = [np.zeros(3), np.array([0.3, -0.2, 0.5])]


@functools.lru_cache(maxsize=None)
def _se3_points():
    out = []
    for th in THETAS:
        for a in AXES:
            for v in TRANSLATIONS:
                out.append(np.concatenate([v, th * a]).astype(np.float32))
    return out


def test_se3_exp_and_so3_exp_within_one_ulp_of_float64(ops):
    """ops.se3_exp and geometry.se3utils.so3_exp at the edges of the small-angle branch ((float)theta < 1e-6f), of the
    polynomial / libm switch of gs_sincos_fast (|x| <= 1) and beyond a full turn: one float32 ulp per entry of the float64
    evaluation rounded once (a zero entry must be zero)."""
    from gradslam_amd.geometry import se3utils
    worst = 0.0
    for xi in _se3_points():
        ref = lm.se3_exp(xi)
        got = host(ops.se3_exp(dev(xi)))
        d = lm.ulp_distance(got, ref)
        got3 = host(se3utils.so3_exp(dev(xi[3:])))
        d3 = lm.ulp_distance(got3, ref[:3, :3])
        worst = max(worst, d.max(), d3.max())
        assert d.max() <= 1.0, (xi, d, got, ref)
        assert d3.max() <= 1.0, (xi, d3, got3, ref[:3, :3])
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], np.float32))
        assert np.array_equal(bits(got[:3, :3]), bits(got3)), "so3_exp is the rotation block of se3_exp"
    print("se3_exp / so3_exp against float64: worst %.2f float32 ulps over %d points" % (worst, len(_se3_points())))


def test_se3_exp_small_angle_rule_sits_on_the_float32_threshold(ops):
    """below (float)1e-6f: R = I + hat(w) exactly and t = R v; from it on: Rodrigues (the diagonal drops below 1 only in
    float64, so the two branches are told apart by the translation)"""
    below, at = _f32_neighbours(1e-6)[0], _f32_neighbours(1e-6)[1]
    v = np.array([0.3, -0.2, 0.5])
    for th, small in ((below, True), (at, False)):
        xi = np.concatenate([v, [0.0, 0.0, th]]).astype(np.float32)
        assert (np.float32(lm.theta_of(xi)) < np.float32(1e-6)) == small
        got = host(ops.se3_exp(dev(xi)))
        assert lm.ulp_distance(got, lm.se3_exp(xi)).max() <= 1.0
        if small:   # no polynomial in this branch: the same float64 operations, so the same bits
            assert np.array_equal(bits(got), bits(lm.se3_exp(xi)))
            w = xi[5]
            assert np.array_equal(got[:3, :3], np.array([[1, -w, 0], [w, 1, 0], [0, 0, 1]], np.float32))
        else:   # V = I + hat(w) / 2 + ...: the translation sits ulps away from the small-angle one
            assert lm.ulp_distance(got[:3, 3], (got[:3, :3].astype(np.float64) @ xi[:3]).astype(np.float32)).max() > 1.0


def _adjoint(xi, Tbar, dt):
    """oracle/icp_backward.se3_exp_adjoint with every operation in the float type `dt` (the oracle's own is float64 only)"""
    xi, Tbar = xi.astype(dt), Tbar.astype(dt)
    one, two, three = dt(1), dt(2), dt(3)
    v, w = xi[:3], xi[3:]
    Rb, tb = Tbar[:3, :3], Tbar[:3, 3]
    wh = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    th = np.sqrt(w @ w)
    small = np.float32(th) < np.float32(1e-6)
    eye = np.eye(3, dtype=dt)
    if small:
        V = eye + wh
    else:
        s, c = np.sin(th), np.cos(th)
        A, Bc, Cc = s / th, (one - c) / (th * th), (th - s) / (th * th * th)
        wh2 = wh @ wh
        V = eye + Bc * wh + Cc * wh2
    vb = V.T @ tb
    Vb = np.outer(tb, v)
    if small:
        whb = Rb + Vb
    else:
        Ab = np.sum(Rb * wh)
        Bb = np.sum(Rb * wh2) + np.sum(Vb * wh)
        Cb = np.sum(Vb * wh2)
        W2b = Bc * Rb + Cc * Vb
        whb = A * Rb + Bc * Vb + W2b @ wh.T + wh.T @ W2b
        dA = (c * th - s) / (th * th)
        dB = (s * th - two * (one - c)) / (th * th * th)
        dC = ((one - c) * th - three * (th - s)) / (th * th * th * th)
        thb = Ab * dA + Bb * dB + Cb * dC
    wb = np.array([whb[2, 1] - whb[1, 2], whb[0, 2] - whb[2, 0], whb[1, 0] - whb[0, 1]], dt)
    if not small:
        wb = wb + thb * w / th
    out = np.concatenate([vb, wb])
    assert out.dtype == dt
    return out


def test_se3_exp_backward_at_the_branch_edges(ops):
    """gs_se3_exp_backward_f32 at the same points against oracle/icp_backward.se3_exp_adjoint (float64), under the bound
    logic of tests/test_hip_backward_kernels.py: KERNEL_FACTOR x the float32-numpy-against-float64-numpy gap of the same
    adjoint on the very input, at least FLOOR_ULPS float32 ulps, every element relative to the largest of the oracle."""
    Tbar32 = np.random.default_rng(11).normal(size=(4, 4)).astype(np.float32)
    Tbar32[3] = 0.0
    worst = 0.0
    for xi in _se3_points():
        ref = ib.se3_exp_adjoint(xi.astype(np.float64), Tbar32.astype(np.float64))
        np.testing.assert_allclose(_adjoint(xi, Tbar32, np.float64), ref, rtol=1e-12, atol=1e-300)
        with np.errstate(all="ignore"):
            gap = bc.rel_err(_adjoint(xi, Tbar32, np.float32), ref)
        bound = bc.kernel_bound(gap if np.isfinite(gap) else 0.0)
        x = dev(xi).requires_grad_(True)
        (ops.se3_exp(x) * dev(Tbar32)).sum().backward()
        got = host(x.grad)
        err = bc.rel_err(got, ref)
        worst = max(worst, err / EPS32)
        print("se3_exp backward xi %s rel %.3e bound %.3e" % (np.array2string(xi, precision=3), err, bound))
        assert np.isfinite(got).all() and err <= bound, (xi, got, ref, err, bound)
    print("se3_exp backward against the float64 adjoint: worst rel %.2f eps32" % worst)


# ------------------------------------------------------------------------------------------------ normal equations
SOLVE_C = 5.0   # sqrt(8) (1 ulp per entry of the rounded AtA, Frobenius against 2-norm) + 1 (Atb) + 1/2 (x rounded), rounded up


def _well_conditioned(rng, rows, ncols):
    q, _ = np.linalg.qr(rng.normal(size=(max(rows, ncols), ncols)))
    return (q[:rows] * np.sqrt(max(rows, ncols)) + 0.1 * rng.normal(size=(rows, ncols))).astype(np.float32)


def _solve_reference(A, b, keep, damp):
    """AtA, Atb in float64, rounded to float32, damp added in float32, solved in float64 (rounded by the caller)"""
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    if keep is not None:
        A64, b64 = A64[keep], b64[keep]
    AtA = (A64.T @ A64).astype(np.float32)
    Atb = (A64.T @ b64).astype(np.float32)
    M = (AtA + np.eye(A.shape[1], dtype=np.float32) * np.float32(damp)).astype(np.float64)
    return np.linalg.solve(M, Atb.astype(np.float64)), float(np.linalg.cond(M))


@pytest.mark.parametrize("damp", [1e-8, 0.5])
@pytest.mark.parametrize("ncols", range(1, 9))
def test_solve_normal_eq_every_column_count_and_row_stride(ops, ncols, damp):
    """gs_solve_normal dispatches on ncols 1..8; the accumulation strides the rows by 256 threads.  Without keep, with a
    random keep and with a keep that leaves exactly ncols rows; |x - ref|_2 <= c eps32 cond(AtA + damp I) |ref|_2 with
    the condition number of the float64 reference (perturbation bound of a linear system whose entries move by an ulp)."""
    worst = 0.0
    for n_rows in (ncols, 255, 256, 257, 1000):
        rng = np.random.default_rng(1000 * ncols + n_rows)
        A = _well_conditioned(rng, n_rows, ncols)
        b = rng.normal(size=n_rows).astype(np.float32)
        exact = np.zeros(n_rows, bool)
        picks = rng.choice(n_rows, ncols, replace=False)
        exact[picks] = True
        A[picks] = _well_conditioned(rng, ncols, ncols)
        rand = rng.random(n_rows) < 0.6
        rand[picks] = True   # (at least the well-conditioned ncols rows: the system stays regular)
        for which, keep in (("all", None), ("random", rand), ("exact", exact)):
            ref, cond = _solve_reference(A, b, keep, damp)
            assert cond < 1e3, (ncols, n_rows, which, cond)
            x = host(ops.solve_normal_eq(dev(A), dev(b), damp=damp,
                                         keep=None if keep is None else torch.from_numpy(keep).cuda()))
            err = np.linalg.norm(x.astype(np.float64) - ref)
            bound = SOLVE_C * EPS32 * cond * np.linalg.norm(ref)
            worst = max(worst, err / (EPS32 * cond * np.linalg.norm(ref)))
            assert x.shape == (ncols,) and np.isfinite(x).all()
            assert err <= bound, (ncols, n_rows, which, damp, err, bound, x, ref)
            xo = o.solve_normal_eq(A, b, damp=damp, keep=keep)   # (the same algorithm, another order of the sums)
            assert np.linalg.norm(x.astype(np.float64) - xo) <= bound, (ncols, n_rows, which, damp, x, xo)
    print("solve_normal_eq ncols %d damp %g: worst %.3f x eps32 cond |x| (c = %g)" % (ncols, damp, worst, SOLVE_C))


# ------------------------------------------------------------------------------------------------ relative pose
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_relative_pose_bit_exact_around_the_block_of_64(ops, n):
    rng = np.random.default_rng(n)

    def poses():
        return np.stack([o.se3_exp(np.concatenate([rng.normal(size=3), rng.normal(size=3) * 0.8]).astype(np.float32))
                         + np.pad(0.01 * rng.normal(size=(3, 4)), ((0, 1), (0, 0))).astype(np.float32)
                         for _ in range(n)])
    T01, T02 = poses(), poses()
    got = host(ops.relative_pose(dev(T01), dev(T02)))
    assert np.array_equal(bits(got), bits(o.relative_pose(T01, T02)))


# ------------------------------------------------------------------------------------------------ (un)projection
def _project_ref(cam, proj, ppm):
    f = np.float32
    out = np.empty((cam.shape[0], 2), np.float32)
    for i in range(cam.shape[0]):
        M = proj[i // ppm]
        p = [cam[i, 0], cam[i, 1], cam[i, 2], cam[i, 3] if cam.shape[1] == 4 else f(1)]
        r = []
        for a in range(3):
            acc = f(M[a, 0] * p[0])
            for k in range(1, 4):
                acc = f(acc + f(M[a, k] * p[k]))
            r.append(acc)
        z = r[2] if r[2] != 0 else f(1)
        out[i] = (f(r[0] / z), f(r[1] / z))
    return out


def _unproject_ref(pix, kinv, depth, ppm):
    f = np.float32
    out = np.empty((pix.shape[0], 3), np.float32)
    for i in range(pix.shape[0]):
        M = kinv[i // ppm]
        p = [pix[i, 0], pix[i, 1], pix[i, 2] if pix.shape[1] == 3 else f(1)]
        for a in range(3):
            acc = f(M[a, 0] * p[0])
            acc = f(acc + f(M[a, 1] * p[1]))
            acc = f(acc + f(M[a, 2] * p[2]))
            out[i, a] = f(acc * depth[i])
    return out


@pytest.mark.parametrize("cdim", [3, 4])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_project_points_bit_exact(ops, n, cdim):
    """100 points per matrix (does not divide the block of 256), one point whose z' is exactly 0 (divided by 1)"""
    rng = np.random.default_rng(10 * n + cdim)
    ppm = 100
    proj = rng.normal(size=((n + ppm - 1) // ppm, 4, 4)).astype(np.float32)
    cam = rng.normal(size=(n, cdim)).astype(np.float32)
    proj[1, 2] = [0.0, 0.0, 1.0, 0.0]
    cam[150, 2] = 0.0
    ref = _project_ref(cam, proj, ppm)
    assert np.array_equal(ref[150], _project_ref(cam[150:151], proj[1:2], ppm)[0]) and np.isfinite(ref).all()
    got = host(ops.project_points(dev(cam), dev(proj), ppm))
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("pdim", [2, 3])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_unproject_points_bit_exact(ops, n, pdim):
    rng = np.random.default_rng(10 * n + pdim)
    ppm = 100
    kinv = rng.normal(size=((n + ppm - 1) // ppm, 3, 3)).astype(np.float32)
    pix = (rng.normal(size=(n, pdim)) * 100).astype(np.float32)
    depth = rng.uniform(0.5, 4.0, n).astype(np.float32)
    got = host(ops.unproject_points(dev(pix), dev(kinv), dev(depth), ppm))
    assert np.array_equal(bits(got), bits(_unproject_ref(pix, kinv, depth, ppm)))
