"""NumPy restatement of the bilateral depth filter (gs_bilateral.hip) and the float64 adjoint of its backward, with the
cases and the committed float32-vs-float64 gaps of the backward tests.  TEST INFRASTRUCTURE ONLY; no test lives here.

Forward (`bilateral`): float32, one rounding per NumPy operation, the exp through `oracle.alpha(..., eps=0.0)` (the
pinned exp of the alpha map) and the sigmas through `oracle.two_sigma_sq`; the window is visited in row-major order
(dy outer, dx inner), which per pixel is the order of the kernel.  The GPU tests compare BITS against it.

Backward (`adjoint`): the formulas of the kernel header evaluated with np.exp in float64 (the reference) or float32 (the
yardstick: `gap = max |f32 - f64| / max |f64|`, tests/backward_cases.py).  The float32 evaluation runs the forward in
float32 too, as the kernel's inputs `out` and `wsum` come from the float32 forward.  Regenerate the gaps:
python -m tests.bilateral_ref"""
import functools

import numpy as np

from oracle import oracle

DEFAULTS = dict(radius=3, sigma_space=2.0, sigma_range=0.03)
# (H, W): 1 pixel, 1 block with a border on every side, one row / column of tiles, odd sizes over several tiles, and
# the 64 x 8 tile exceeded by one pixel in each direction
SIZES = [(1, 1), (2, 2), (2, 300), (300, 2), (67, 131), (9, 65)]
RADII = [0, 1, 3, 8]
BACKWARD_CASES = [(H, W, r) for H, W in SIZES for r in (1, 3, 8)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _shift(a, dy, dx, fill=0.0):
    """b[h, w] = a[h + dy, w + dx], `fill` outside the image"""
    H, W = a.shape
    b = np.full_like(a, fill)
    h0, h1 = max(0, -dy), min(H, H - dy)
    w0, w1 = max(0, -dx), min(W, W - dx)
    if h0 < h1 and w0 < w1:
        b[h0:h1, w0:w1] = a[h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return b


def bilateral(depth, radius=3, sigma_space=2.0, sigma_range=0.03):
    """depth (H, W) float32 -> (out, wsum) float32: the arithmetic contract of gs_bilateral_depth_f32."""
    d = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = d.shape
    with np.errstate(invalid="ignore"):
        centre = d > 0
    S = np.zeros((H, W), np.float32)
    Wt = np.zeros((H, W), np.float32)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            dp = _shift(d, dy, dx)
            with np.errstate(invalid="ignore"):
                use = centre & (dp > 0)
            g = oracle.alpha(np.array([[dx, dy, 0]], np.float32), sigma_space, eps=0.0)[0]
            diff = np.where(use, dp - np.where(centre, d, np.float32(0)), np.float32(0)).astype(np.float32)
            pts = np.zeros((H, W, 3), np.float32)
            pts[..., 0] = diff
            e = oracle.alpha(pts, sigma_range, eps=0.0)
            w = (np.float32(g) * e).astype(np.float32)
            t = (w * np.where(use, dp, np.float32(0))).astype(np.float32)
            S = np.where(use, S + t, S).astype(np.float32)
            Wt = np.where(use, Wt + w, Wt).astype(np.float32)
    out = d.copy()
    out[centre] = (S[centre] / Wt[centre]).astype(np.float32)
    return out, Wt


def bilateral_stack(depth, **kw):
    d = np.asarray(depth, np.float32)
    flat = d.reshape((-1,) + d.shape[-2:])
    res = [bilateral(f, **kw) for f in flat]
    return (np.stack([r[0] for r in res]).reshape(d.shape), np.stack([r[1] for r in res]).reshape(d.shape))


# ------------------------------------------------------------------------------------------ float64 forward / adjoint
def _weights(d, valid, radius, sigma_space, sigma_range, dtype):
    """per offset (dy, dx): (neighbour depth, w) with w = 0 where the pair is not used"""
    two_s = dtype(oracle.two_sigma_sq(sigma_space))
    two_r = dtype(oracle.two_sigma_sq(sigma_range))
    dz = np.where(valid, d, dtype(0))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            dp = _shift(dz, dy, dx)
            use = valid & _shift(valid, dy, dx, fill=False)
            diff = np.where(use, dp - dz, dtype(0))
            w = np.where(use, np.exp(-dtype(dx * dx + dy * dy) / two_s) * np.exp(-(diff * diff) / two_r), dtype(0))
            yield dy, dx, dp, diff, w.astype(dtype)


def forward_np(depth, radius=3, sigma_space=2.0, sigma_range=0.03, dtype=np.float64):
    """the filter with np.exp in `dtype` (depth may be float64: finite differences) -> (out, wsum)"""
    d = np.asarray(depth).astype(dtype)
    with np.errstate(invalid="ignore"):
        valid = d > 0
    S = np.zeros(d.shape, dtype)
    Wt = np.zeros(d.shape, dtype)
    for _, _, dp, _, w in _weights(d, valid, radius, sigma_space, sigma_range, dtype):
        S = S + w * dp
        Wt = Wt + w
    out = d.copy()
    out[valid] = S[valid] / Wt[valid]
    return out, Wt


def adjoint(depth, out_bar, radius=3, sigma_space=2.0, sigma_range=0.03, dtype=np.float64):
    """depth_bar of sum(out * out_bar) by the formulas of gs_bilateral.hip, everything in `dtype`:
        centre q, neighbour p = q + o, o != 0:   bar[p] += ob_q (w / W_q) (1 - c),   bar[q] += ob_q (w / W_q) c
        with c = (d_p - out_q)(d_p - d_q) / sigma_range^2;   bar[q] += ob_q / W_q (the centre's own weight is 1);
        invalid pixels: bar = ob."""
    d = np.asarray(depth).astype(dtype)
    ob = np.asarray(out_bar).astype(dtype)
    with np.errstate(invalid="ignore"):
        valid = d > 0
    out, Wt = forward_np(d, radius, sigma_space, sigma_range, dtype)
    sr2 = dtype(oracle.two_sigma_sq(sigma_range)) / dtype(2)
    k = np.where(valid, ob / np.where(valid, Wt, dtype(1)), dtype(0))     # ob_q / W_q
    oz = np.where(valid, out, dtype(0))
    bar = k.copy()
    for dy, dx, dp, diff, w in _weights(d, valid, radius, sigma_space, sigma_range, dtype):
        if dy == 0 and dx == 0:
            continue
        c = (dp - oz) * diff / sr2
        bar = bar + k * w * c                                   # to the centre q
        bar = bar + _shift(k * w * (dtype(1) - c), -dy, -dx)    # to the neighbour p = q + o
    return np.where(valid, bar, ob).astype(dtype)


# ------------------------------------------------------------------------------------------ cases
def plane_scene(H=48, W=64, fx=60.0, noise=0.004, holes=0.05, seed=0):
    """(clean depth, noisy depth with holes, K): an inclined plane with a 0.8 m step at the middle column."""
    w, h = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    clean = 1.5 + 0.004 * w + 0.006 * h + np.where(w >= W // 2, 0.8, 0.0)
    rng = np.random.default_rng([7, H, W, seed])
    noisy = clean + noise * rng.standard_normal((H, W))
    noisy[rng.random((H, W)) < holes] = 0.0
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = fx
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return clean.astype(np.float32), noisy.astype(np.float32), K


@functools.lru_cache(maxsize=None)
def case(H, W, seed=0):
    """(H, W) float32 depth, deterministic: the noisy stepped plane with 5 % holes, an invalid last column and last
    row (where the image has more than two of them) and, from 64 pixels on, a negative and a NaN pixel with valid
    neighbours.  Read-only."""
    _, d, _ = plane_scene(H, W, seed=seed)
    if W > 2:
        d[:, W - 1] = 0.0
    if H > 2:
        d[H - 1, :] = 0.0
    if H * W >= 64:
        hn, wn = (H // 2 if H > 2 else 0), (W // 3 if W > 2 else 0)
        hq, wq = (H // 3 if H > 2 else 0), (W // 2 if W > 2 else 0)
        d[hn, wn] = -1.25
        d[hq, wq] = np.nan
        if W > 2:      # (valid neighbours on both sides of the NaN)
            d[hq, wq - 1] = d[hq, wq + 1] = 2.0
        else:
            d[hq - 1, wq] = d[hq + 1, wq] = 2.0
    else:
        d.flat[0] = 1.5
    d.setflags(write=False)
    return d


def weights(H, W, seed=11):
    return np.random.default_rng([seed, H, W]).standard_normal((H, W)).astype(np.float32)


def backward_key(H, W, radius):
    return "%dx%d/r%d" % (H, W, radius)


def backward_gap(H, W, radius):
    from tests import backward_cases as bc
    d, ob = case(H, W), weights(H, W)
    kw = dict(DEFAULTS, radius=radius)
    return bc.rel_err(adjoint(d, ob, dtype=np.float32, **kw), adjoint(d, ob, **kw))


# (float32 numpy against float64 numpy, CPU; two significant digits)
# GAPS-BEGIN
BACKWARD_GAP = {
    '1x1/r1': 0.0e+00,
    '1x1/r3': 0.0e+00,
    '1x1/r8': 0.0e+00,
    '2x2/r1': 1.3e-06,
    '2x2/r3': 1.3e-06,
    '2x2/r8': 1.3e-06,
    '2x300/r1': 2.3e-06,
    '2x300/r3': 3.4e-06,
    '2x300/r8': 3.7e-06,
    '300x2/r1': 2.2e-06,
    '300x2/r3': 4.7e-06,
    '300x2/r8': 7.6e-06,
    '67x131/r1': 4.1e-06,
    '67x131/r3': 4.3e-06,
    '67x131/r8': 1.2e-05,
    '9x65/r1': 2.9e-06,
    '9x65/r3': 4.0e-06,
    '9x65/r8': 2.3e-05,
}
# GAPS-END


if __name__ == "__main__":
    print("BACKWARD_GAP = {")
    for H, W, r in BACKWARD_CASES:
        print("    %r: %.1e," % (backward_key(H, W, r), backward_gap(H, W, r)))
    print("}")
