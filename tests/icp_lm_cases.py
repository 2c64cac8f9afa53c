"""Small seeded scenes for the scalar stage of the ICP solve, each with the regime it has to reach.

A scene is a bumpy patch z = 0.4 sin(2.5 u) cos(2 v) + 0.3 u v sampled at random (u, v) as targets with analytic normals,
and other samples of it, rotated about a random axis and shifted, as the source; `tiny_theta` is a flat plane whose
source is translated and tilted by 1e-4 rad.  Every case carries a witness: a predicate over a (K, 12) trace
[err, new_err, damp_after, sigmoid, xi(6), 0, 0] that holds only if the run visited the regime the case is named for.
tests/test_icp_lm_cpu.py proves each witness (and the decisiveness margin of the cases marked decisive) on the CPU
oracle's trace; tests/test_hip_icp_lm.py asserts it again on the kernels' own traces.

Sizes: 96 points run the brute-force driver, 640 points the grid driver (its row unit is 96 points: six full units and
one of 64)."""
import functools

import numpy as np

from tests import icp_lm_ref as lm

N_BRUTE, N_GRID = 96, 640
DECISIVE_MARGIN = 1e-3      # |new_err - err| >= 1e-3 err: ten times the rtol = 1e-4 the parity test allows on err


def _patch(uv):
    u, v = uv[:, 0], uv[:, 1]
    z = 0.4 * np.sin(2.5 * u) * np.cos(2.0 * v) + 0.3 * u * v
    zu = 1.0 * np.cos(2.5 * u) * np.cos(2.0 * v) + 0.3 * v
    zv = -0.8 * np.sin(2.5 * u) * np.sin(2.0 * v) + 0.3 * u
    n = np.stack([-zu, -zv, np.ones_like(u)], 1)
    return np.stack([u, v, z], 1), n / np.linalg.norm(n, axis=1, keepdims=True)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def scene(kind, seed, n, angle, shift, scale):
    """(src (n, 3), tgt (n, 3), tgt_normals (n, 3)) float32; read-only (shared between tests)"""
    rng = np.random.default_rng(seed)
    uv_t, uv_s = rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(-0.8, 0.8, (n, 2))
    axis, tdir = rng.normal(size=3), rng.normal(size=3)
    if kind == "patch":
        tgt, tn = _patch(uv_t)
        p, _ = _patch(uv_s)
        R = _rotation(axis, angle)
        c = p.mean(0)
        src = (p - c) @ R.T + c + shift * tdir / np.linalg.norm(tdir)
    else:   # "plane": z = 0 seen from a source that is translated and tilted by `angle` about an in-plane axis
        tgt = np.concatenate([uv_t, np.zeros((n, 1))], 1)
        tn = np.tile([0.0, 0.0, 1.0], (n, 1))
        p = np.concatenate([uv_s, np.zeros((n, 1))], 1)
        src = p @ _rotation([1.0, 0.5, 0.0], angle).T + shift * np.array([0.3, -0.2, 1.0])
    out = tuple(np.ascontiguousarray(a * (scale if i < 2 else 1.0), dtype=np.float32)
                for i, a in enumerate((src, tgt, tn)))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- trace helpers
def pattern(trace):
    """'A' / 'R' per iteration: the mode-0 decision new_err < err"""
    return "".join("A" if r[1] < r[0] else "R" for r in np.asarray(trace, np.float32))


def margins(trace):
    t = np.asarray(trace, np.float64)
    return np.abs(t[:, 1] - t[:, 0]) / t[:, 0]


def thetas(trace, prm):
    """theta of every se3_exp the stage evaluates: of xi (the look-ahead transform) and, in mode 1, of sig * xi"""
    t = np.asarray(trace, np.float32)
    th = [lm.theta_of(r[4:10]) for r in t]
    if prm["mode"] == 1:
        th += [lm.theta_of((r[3] * r[4:10]).astype(np.float32)) for r in t]
    return np.array(th)


def errdiffs(trace):
    t = np.asarray(trace, np.float32)
    return (t[:, 1] - t[:, 0]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- witnesses
def w_decisive0(trace, prm):
    p = pattern(trace)
    return p.count("A") >= 3 and p.count("R") >= 3


def w_reaccept(trace, prm):
    p = pattern(trace)
    return w_decisive0(trace, prm) and "RA" in p


def w_soft_mid(trace, prm):
    """some iteration has sig and the damping factor well inside (0, 1) and (lmin, lambda_max)"""
    lmin, lrange = (float(x) for x in lm.soft_constants(prm))
    ok = False
    for k, r in enumerate(np.asarray(trace, np.float32)):
        f, s = lm.soft_factor(r[0], r[1], prm)
        ok |= (lmin + 0.1 * lrange < float(f) < lmin + 0.9 * lrange) and (0.1 < float(s) < 0.9)
    return ok


def w_clamp_lo(trace, prm):
    return bool((errdiffs(trace) < -70.0).any())


def w_clamp_hi(trace, prm):
    return bool((errdiffs(trace) > 70.0).any())


def w_saturate(trace, prm):
    """-B * errdiff (errdiff clamped) beyond 700: gs_exp_fast's libm fall-back, whose result overflows float32"""
    d = np.clip(errdiffs(trace), -70.0, 70.0).astype(np.float64)
    return bool((-float(np.float32(prm["B"])) * d > 700.0).any())


def w_tiny_theta(trace, prm):
    th = thetas(trace, prm).astype(np.float32)
    return bool((th < np.float32(1e-6)).any() and (th >= np.float32(1e-6)).any())


def w_big_theta(trace, prm):
    return bool((thetas(trace, prm) > 1.0).any())


DEFAULT = dict(damp=1e-8, lambda_max=2.0, B=1.0, B2=1.0, nu=200.0)
SOFT = dict(damp=1e-3, lambda_max=5.0, B=3.0, B2=0.5, nu=2.0)
ITERS = 12
SIZES = (N_BRUTE, N_GRID)


def _case(name, witness, witness_modes, at, kind="patch", shift=0.3, scale=1.0, decisive=None, **over):
    """at: per size, the seed and the rotation angle of the scene (and parameter overrides, if any); decisive: per size,
    the modes in which every iteration clears DECISIVE_MARGIN on the oracle's trace"""
    return dict(name=name, kind=kind, shift=shift, scale=scale, iters=ITERS, prm=dict(DEFAULT, **over), at=at,
                witness=witness, witness_modes=witness_modes, decisive=decisive or {N_BRUTE: (), N_GRID: ()})


# Seeds, angles and the initial damping were chosen with the CPU oracle alone; tests/test_icp_lm_cpu.py holds every one
# of them to its witness at both sizes, and the decisive ones to DECISIVE_MARGIN.  A case names the modes its witness is
# about; the GPU tests run every case in both modes and assert the witness in those.
CASES = [
    # (a) hard LM with a clear margin on every decision: accepts, then rejects
    _case("decisive0", w_decisive0, (0,), {N_BRUTE: dict(seed=13, angle=0.3), N_GRID: dict(seed=25, angle=0.3)},
          decisive={N_BRUTE: (0, 1), N_GRID: (0, 1)}),
    # (a) ... and an accept after a run of rejects (a larger initial damping, so that doubling it matters)
    _case("reaccept", w_reaccept, (0,), {N_BRUTE: dict(seed=84, angle=0.3, damp=0.1),
                                         N_GRID: dict(seed=86, angle=0.9, damp=1.0)},
          decisive={N_BRUTE: (0, 1), N_GRID: (0,)}),
    # (b) gradLM away from its defaults: sig and the damping factor in the middle of their ranges
    _case("soft_mid", w_soft_mid, (1,), {N_BRUTE: dict(seed=54, angle=0.9), N_GRID: dict(seed=58, angle=0.3)},
          decisive={N_BRUTE: (0, 1), N_GRID: (0, 1)}, **SOFT),
    # (c) the scene scaled up: the error difference runs into the clamp at -70 ...
    _case("clamp_lo", w_clamp_lo, (1,), {N_BRUTE: dict(seed=0, angle=0.3), N_GRID: dict(seed=0, angle=0.3)}, scale=5.0),
    # (c) ... and, when the first step overshoots, into the one at +70
    _case("clamp_hi", w_clamp_hi, (1,), {N_BRUTE: dict(seed=9, angle=1.2, scale=5.0),
                                         N_GRID: dict(seed=25, angle=1.2, scale=10.0)},
          decisive={N_BRUTE: (1,), N_GRID: (1,)}),
    # (d) B and B2 large: B * 70 > 700, libm's exp; the exponential overflows float32, the factor is lmin, sig is 0
    _case("saturate", w_saturate, (1,), {N_BRUTE: dict(seed=9, angle=1.2, scale=5.0),
                                         N_GRID: dict(seed=25, angle=1.2, scale=10.0)}, B=20.0, B2=15.0),
    # (e) a plane seen from a translated, 1e-4 rad tilted source: theta above 1e-6 first, below it once converged
    _case("tiny_theta", w_tiny_theta, (0, 1), {N_BRUTE: dict(seed=0, angle=1e-4), N_GRID: dict(seed=1, angle=1e-4)},
          kind="plane", shift=0.1),
    # (f) a rotation of more than a radian in one step: libm's sin / cos instead of the polynomials
    _case("big_theta", w_big_theta, (0, 1), {N_BRUTE: dict(seed=7, angle=1.2), N_GRID: dict(seed=23, angle=1.2)},
          decisive={N_BRUTE: (0, 1), N_GRID: (0, 1)}),
]
BY_NAME = {c["name"]: c for c in CASES}
_SCENE_KEYS = ("seed", "angle", "scale")


def params(case, n, mode):
    """the ICP parameters of the case at n points, in the given mode"""
    p = dict(case["prm"], mode=mode)
    p.update({k: v for k, v in case["at"][n].items() if k not in _SCENE_KEYS})
    return p


def clouds(case, n):
    at = case["at"][n]
    return scene(case["kind"], at["seed"], n, at["angle"], case["shift"], at.get("scale", case["scale"]))


def icp_kwargs(case, n, mode):
    p = params(case, n, mode)
    return dict(mode=mode, numiters=case["iters"], damp=p["damp"], lambda_max=p["lambda_max"], B=p["B"], B2=p["B2"],
                nu=p["nu"])


@functools.lru_cache(maxsize=None)
def _oracle_run(name, n, mode):
    from oracle import oracle as o
    case = BY_NAME[name]
    src, tgt, tn = clouds(case, n)
    T, _, tr = o.icp(src, tgt, tn, return_trace=True, **icp_kwargs(case, n, mode))
    T.setflags(write=False)
    tr.setflags(write=False)
    return T, tr


def oracle_run(case, n, mode):
    """(T, trace) of the CPU oracle on the case at n points, computed once and shared (read-only)"""
    return _oracle_run(case["name"], n, mode)
