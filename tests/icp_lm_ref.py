"""NumPy restatement of the scalar stage of an ICP iteration: the hard-LM accept / reject, the gradLM soft update, the
SE(3) exponential and the 4x4 accumulation into the pose.  Restated from oracle/gs_oracle.c (icp_impl, gs_or_se3_exp,
mm4), cast for cast: every float32 value is a numpy float32, every float64 value a Python float, and the transcendental
functions are libm's (the math module), the ones the oracle links against.  tests/test_icp_lm_cpu.py proves it against
the oracle bit for bit before tests/test_hip_icp_lm.py points it at the kernels.

A trace is the (K, 12) float32 array every ICP entry point records: [err, new_err, damp_after, sigmoid, xi(6), 0, 0].
`prm` is a dict with the keys mode, damp, lambda_max, B, B2, nu (numiters is the length of the trace)."""
import math

import numpy as np

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)   # 2^-23: the largest relative distance between neighbouring float32


def _f32(x):
    """one rounding of a float64 to float32 (overflow gives inf, as the C cast does)"""
    with np.errstate(over="ignore"):
        return np.float32(x)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _pow(x, y):
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf


def theta_of(xi):
    """the rotation angle as se3_exp sees it: float64 norm of the float32 rotation part"""
    w = [float(f32(c)) for c in np.asarray(xi).reshape(6)[3:]]
    return math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])


def so3_exp(w32):
    """3x3 rotation of se3_exp (float64 inside, rounded once)"""
    xi = np.zeros(6, np.float32)
    xi[3:] = np.asarray(w32, np.float32).reshape(3)
    return se3_exp(xi)[:3, :3].copy()


def se3_exp(xi32):
    """(4, 4) float32: geometry/se3utils.py:77-115 in float64 from the float32 xi, rounded once.  (float)theta < 1e-6f
    takes R = I + hat(w) and V = R.  Operation order of gs_or_se3_exp."""
    xi = [float(f32(c)) for c in np.asarray(xi32).reshape(6)]
    v, w = xi[:3], xi[3:]
    wh = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    eye = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    if f32(theta) < f32(1e-6):
        R = [eye[i] + wh[i] for i in range(9)]
        V = list(R)
    else:
        wh2 = [0.0] * 9
        for i in range(3):
            for j in range(3):
                s = 0.0
                for k in range(3):
                    s += wh[3 * i + k] * wh[3 * k + j]
                wh2[3 * i + j] = s
        s, c = math.sin(theta), math.cos(theta)
        Ac, Bc, Cc = s / theta, (1 - c) / (theta * theta), (theta - s) / (theta * theta * theta)
        R = [eye[i] + Ac * wh[i] + Bc * wh2[i] for i in range(9)]
        V = [eye[i] + Bc * wh[i] + Cc * wh2[i] for i in range(9)]
    T = np.zeros((4, 4), np.float32)
    for i in range(3):
        for j in range(3):
            T[i, j] = _f32(R[3 * i + j])
        T[i, 3] = _f32(V[3 * i] * v[0] + V[3 * i + 1] * v[1] + V[3 * i + 2] * v[2])
    T[3, 3] = 1.0
    return T


def compose(T_step, T_total):
    """T_step . T_total as the 4x4 float32 product of mm4: plain multiply / add, k ascending, no FMA"""
    A, B = np.asarray(T_step, np.float32), np.asarray(T_total, np.float32)
    C = np.empty((4, 4), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(4):
            for j in range(4):
                acc = f32(A[i, 0] * B[0, j])
                for k in range(1, 4):
                    acc = f32(acc + f32(A[i, k] * B[k, j]))
                C[i, j] = acc
    return C


def hard_update(err, new_err, damp):
    """mode 0: (damp_after, accepted).  Halving and doubling are exact in float32."""
    err, new_err, damp = f32(err), f32(new_err), f32(damp)
    if new_err < err:
        return f32(damp / f32(2)), True
    return f32(damp * f32(2)), False


def soft_constants(prm):
    lmax = float(f32(prm["lambda_max"]))
    return _f32(1.0 / lmax), _f32(lmax - 1.0 / lmax)


def clamp_errdiff(err, new_err):
    d = f32(f32(new_err) - f32(err))
    return f32(-70.0) if d < f32(-70.0) else (f32(70.0) if d > f32(70.0) else d)


def soft_factor(err, new_err, prm):
    """mode 1: (damping factor, sig) of one iteration, the casts of gs_or_icp"""
    lmin, lrange = soft_constants(prm)
    d = clamp_errdiff(err, new_err)
    with np.errstate(over="ignore", invalid="ignore"):
        e_b = _f32(_exp(float(f32(_f32(-float(f32(prm["B"]))) * d))))
        factor = f32(lmin + f32(lrange / f32(f32(1.0) + e_b)))
        e_b2 = _f32(_exp(float(f32(_f32(-float(f32(prm["B2"]))) * d))))
        pw = _f32(_pow(float(f32(f32(1.0) + e_b2)), float(_f32(1.0 / float(f32(prm["nu"]))))))
        sig = f32(f32(1.0) / pw)
    return factor, sig


def soft_update(err, new_err, damp, prm):
    """mode 1: (damp_after, sig)"""
    factor, sig = soft_factor(err, new_err, prm)
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(damp) * factor), sig


def soft_formulas_f64(d, prm):
    """(damping factor, sig) of the float64 formula at errdiff d (already clamped); both are monotone in d"""
    lmax = float(f32(prm["lambda_max"]))
    lmin, lrange = 1.0 / lmax, lmax - 1.0 / lmax
    B, B2, nu = float(f32(prm["B"])), float(f32(prm["B2"])), float(f32(prm["nu"]))
    factor = lmin + lrange / (1.0 + _exp(-B * d))
    sig = 1.0 / _pow(1.0 + _exp(-B2 * d), 1.0 / nu)
    return factor, sig


def replay(trace, prm, init=None):
    """Rebuilds damp, sig, T_step of every iteration and the final T from the err, new_err and xi columns of a trace
    alone.  Returns a dict: damp (K,), sig (K,), factor (K,) (mode 1: damp_k / damp_{k-1} as computed), accept (K,) bool
    (mode 1: all True), T_step (K, 4, 4), T (4, 4)."""
    trace = np.asarray(trace, np.float32)
    K = trace.shape[0]
    T = np.eye(4, dtype=np.float32) if init is None else np.array(init, np.float32).reshape(4, 4)
    damp = f32(prm["damp"])
    out = dict(damp=np.zeros(K, np.float32), sig=np.ones(K, np.float32), factor=np.ones(K, np.float32),
               accept=np.ones(K, bool), T_step=np.zeros((K, 4, 4), np.float32))
    for k in range(K):
        err, new_err, xi = trace[k, 0], trace[k, 1], trace[k, 4:10]
        if prm["mode"] == 0:
            damp, acc = hard_update(err, new_err, damp)
            out["accept"][k] = acc
            out["factor"][k] = 0.5 if acc else 2.0
            step = se3_exp(xi) if acc else np.eye(4, dtype=np.float32)
            if acc:
                T = compose(step, T)
        else:
            factor, sig = soft_factor(err, new_err, prm)
            with np.errstate(over="ignore", invalid="ignore"):
                damp = f32(damp * factor)
                xs = (sig * xi).astype(np.float32)
            out["factor"][k], out["sig"][k] = factor, sig
            step = se3_exp(xs)
            T = compose(step, T)
        out["damp"][k] = damp
        out["T_step"][k] = step
    out["T"] = T
    return out


def ulp_distance(got, ref):
    """per element |got - ref| in units of the float32 spacing at ref (0 where the bits agree or both are zero; inf
    where exactly one of them is not finite)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    same = (got.view(np.int32) == ref.view(np.int32)) | ((got == 0) & (ref == 0))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    d = np.where(np.isfinite(d), d, np.inf)
    return np.where(same, 0.0, d)
