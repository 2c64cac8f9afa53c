"""CPU: the references that tests/test_hip_ingest_stream.py holds the ingest kernels to, on the cases of
tests/ingest_cases.py.

  * oracle.ingest_depth / oracle.ingest_color (the restatement of OpenCV's resize arithmetic, which the resize kernels must
    equal bit for bit) against an independent statement of the same operation written pixel by pixel in float64 / exact
    integers: nearest neighbour by floor(dst * src / dst) -- bit for bit --, pixel-centre bilinear interpolation with the
    clamp at both borders -- within the bound derived in ingest_cases.color_bound(), which is far below what a resize that
    is one source pixel off changes;
  * the float64 statement of the native conversion, (raw / div) cast last, against the oracle at the same size: after
    this the GPU tests have ONE reference, and the per-frame and the one-launch entry points are tied together;
  * that the case families are what they say: pixel counts on both sides of one block and of one sweep of the capped grid
    for every modality mix, planted extremes where they belong, streamer content that tells every (t, b) apart."""
import math

import numpy as np
import pytest

from oracle import oracle as o
from tests import ingest_cases as ic


# ------------------------------------------------------------------------------------------------ resize
def nn_index(d, n_dst, n_src):
    return min((d * n_src) // n_dst, n_src - 1)           # floor(d * n_src / n_dst), exactly


def lin_taps(n_dst, n_src):
    """per destination index: (s0, s1, f) of pixel-centre linear interpolation, clamped with weight 0 at both borders"""
    taps = []
    for d in range(n_dst):
        x = (d + 0.5) * n_src / n_dst - 0.5
        s = math.floor(x)
        f = x - s
        if s < 0:
            s, f = 0, 0.0
        if s >= n_src - 1:
            s, f = n_src - 1, 0.0
        taps.append((s, min(s + 1, n_src - 1), f))
    return taps


def bilinear_f64(raw, H, W):
    raw = raw.astype(np.float64)
    H0, W0 = raw.shape[:2]
    ty, tx = lin_taps(H, H0), lin_taps(W, W0)
    y0, y1, fy = (np.array([t[k] for t in ty]) for k in range(3))
    x0, x1, fx = (np.array([t[k] for t in tx]) for k in range(3))
    fy, fx = fy[:, None, None], fx[None, :, None]
    g = lambda ys, xs: raw[ys[:, None], xs[None, :]]      # noqa: E731
    return (1 - fy) * (1 - fx) * g(y0, x0) + (1 - fy) * fx * g(y0, x1) + fy * (1 - fx) * g(y1, x0) + fy * fx * g(y1, x1)


@pytest.mark.parametrize("case", ic.RESIZE_CASES, ids=ic.resize_name)
def test_oracle_depth_resize_is_nearest_neighbour_by_floor(case):
    (H0, W0), (H, W) = case
    raw, _ = ic.resize_source(H0, W0)
    want = np.empty((H, W), np.uint16)
    for y in range(H):
        sy = nn_index(y, H, H0)
        for x in range(W):
            want[y, x] = raw[sy, nn_index(x, W, W0)]
    for div in ic.RESIZE_SCALE_DIVS:
        got = o.ingest_depth(raw, H, W, div)
        assert got.dtype == np.float32 and got.shape == (H, W)
        assert np.array_equal(got.view(np.int32), ic.native_depth_ref(want, div).view(np.int32)), div
    # the corners of the source are the corners' nearest neighbours at the top left, and the last row / column is reached
    # only where the target is at least as large
    assert want[0, 0] == raw[0, 0]
    if H >= H0 and W >= W0:
        assert want[-1, -1] == raw[-1, -1]


def test_nearest_neighbour_clamp_is_never_reached():
    """floor(d * (1 / (n_dst / n_src))) < n_src for every d < n_dst: the float64 product is below n_src by n_src / n_dst,
    far more than its rounding.  The clamp to n_src - 1 (OpenCV's, kept in the oracle and the kernel) is a safety net that
    no case can exercise -- a kernel whose clamp is off by one gives the same pixels.  (The rounded product may fall BELOW
    an integer that the exact quotient reaches, e.g. 49 * (1 / (98 / 2)) < 1: there OpenCV's arithmetic, which the oracle
    restates, picks the pixel before; none of the resize cases has such a pixel, the test above would show it.)"""
    below = 0
    for n_src in (1, 2, 3, 5, 7, 23, 24, 31, 32, 480, 640):
        for n_dst in list(range(1, 130)) + [240, 320, 480, 640, 1920]:
            d = np.arange(n_dst)
            s = np.floor(d * (1.0 / (n_dst / n_src))).astype(np.int64)
            exact = (d * n_src) // n_dst
            assert 0 <= s.min() and s.max() <= n_src - 1 and (s <= exact).all() and (s >= exact - 1).all(), (n_src, n_dst)
            below += int((s < exact).sum())
    assert below > 0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("case", ic.RESIZE_CASES, ids=ic.resize_name)
def test_oracle_colour_resize_is_bilinear_within_the_derived_bound(case, normalize):
    (H0, W0), (H, W) = case
    _, raw = ic.resize_source(H0, W0)
    want = bilinear_f64(raw, H, W)
    if normalize:
        want = want / 255.0
    got = o.ingest_color(raw, H, W, normalize)
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    bound = ic.COLOR_BOUNDS[ic.resize_name(case)][int(normalize)]
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s normalize=%d: max |oracle - float64| = %.3e, bound %.3e" % (ic.resize_name(case), normalize, err, bound))
    assert err <= bound
    # tight enough to notice a resize that is one source pixel off: far below the smallest planted neighbour difference
    step = ic.planted_step(raw) / (255.0 if normalize else 1.0)
    assert bound < 1e-3 * step
    if (H, W) == (H0, W0):       # a copy
        assert np.array_equal(got, ic.native_color_ref(raw, normalize))


def test_one_pixel_shift_breaks_the_colour_bound():
    """the bound does its job: the float64 interpolation of the source shifted by one pixel along either axis misses the
    oracle by far more than the bound, on the planted last row / column"""
    case = ((23, 31), (37, 53))
    _, raw = ic.resize_source(*case[0])
    got = o.ingest_color(raw, *case[1]).astype(np.float64)
    for axis in (0, 1):
        shifted = bilinear_f64(np.roll(raw, 1, axis=axis), *case[1])
        assert np.abs(got - shifted).max() > 100 * ic.COLOR_BOUNDS[ic.resize_name(case)][0]


def test_resize_cases_cover_what_they_claim():
    cases = set(ic.RESIZE_CASES)
    assert {c[0] for c in cases} == {(1, 1), (1, 7), (5, 1), (2, 3), (23, 31), (24, 32)}
    for src in {c[0] for c in cases}:
        assert (src, src) in cases and (src, (1, 1)) in cases
    for need in (((23, 31), (23, 40)), ((23, 31), (9, 31)), ((23, 31), (37, 53)), ((23, 31), (10, 7)), ((2, 3), (240, 320))):
        assert need in cases
    assert any(h % h0 == 0 and w % w0 == 0 and (h, w) != (h0, w0) and h0 * w0 > 1 for (h0, w0), (h, w) in cases)   # integer up
    assert any(h0 % h == 0 and w0 % w == 0 and (h, w) not in ((h0, w0), (1, 1)) for (h0, w0), (h, w) in cases)       # integer down
    assert 240 * 320 > 256
    for (h0, w0) in {c[0] for c in cases}:
        d, c = ic.resize_source(h0, w0)
        assert {int(d[y, x]) for y in (0, -1) for x in (0, -1)} <= set(ic.DEPTH_PLANT)
        assert {int(v) for y in (0, -1) for x in (0, -1) for v in c[y, x]} <= set(ic.COLOR_PLANT)
        if w0 >= 5:
            assert set(ic.DEPTH_PLANT) <= {int(v) for v in d[-1]} and set(ic.COLOR_PLANT) <= {int(v) for v in c[-1, :, 0]}
        if h0 >= 5:
            assert set(ic.DEPTH_PLANT) <= {int(v) for v in d[:, -1]} and set(ic.COLOR_PLANT) <= {int(v) for v in c[:, -1, 0]}
        if h0 * w0 > 1:
            assert ic.planted_step(c) == 255.0 and ic.planted_step(d) >= 1.0


# ------------------------------------------------------------------------------------------------ native conversion
@pytest.mark.parametrize("shape", ic.NATIVE_SHAPES, ids=ic.native_name)
def test_native_reference_equals_the_oracle_at_the_same_size(shape):
    n, H, W = shape
    d, c = ic.native_raw(shape)
    for div in ic.NATIVE_SCALE_DIVS:
        want = ic.native_depth_ref(d, div)
        assert want.dtype == np.float32
        for i in (0, n - 1):
            assert np.array_equal(want[i].view(np.int32), o.ingest_depth(d[i], H, W, div).view(np.int32))
    for normalize in (False, True):
        want = ic.native_color_ref(c, normalize)
        for i in (0, n - 1):
            assert np.array_equal(want[i].view(np.int32), o.ingest_color(c[i], H, W, normalize).view(np.int32))
    # a signed reading of the depth would differ: values at or above 32768 are there, in every position of a quad
    flat = d.reshape(-1)
    if flat.size >= 40:
        for k in range(4):          # every planted value in every position of a quad, at both ends
            assert set(ic.DEPTH_PLANT) == set(flat[k:20:4].tolist()) == set(flat[flat.size - 20 + k::4].tolist())
    else:
        assert (flat >= 32768).any() and (flat < 32768).any()


def test_native_pixel_counts_sit_on_both_sides_of_every_launch_constant():
    T, S, P = ic.THREADS, ic.SWEEP, ic.PX_PER_ITEM
    assert S == T * ic.BLOCKS and P == 4
    px = sorted({n * h * w for n, h, w in ic.NATIVE_SHAPES})
    assert {P, T - P, T, T + P} <= set(px)
    items = {"both": lambda p: p, "color": lambda p: 3 * p // 4, "depth": lambda p: p // 4}
    for mode, f in items.items():
        it = sorted(f(p) for p in px)
        below = [i for i in it if i < S]
        above = [i for i in it if i > S]
        assert below and S - max(below) <= P and above and min(above) - S <= P, mode     # the nearest counts to one sweep
        assert max(it) > 2 * S, mode
        if S % {"both": 1, "color": 3, "depth": 1}[mode] == 0:
            assert S in it, mode
    assert (4, 3, 5) in ic.NATIVE_SHAPES
    assert set(ic.NATIVE_SCALE_DIVS) == {5000.0, 1000.0, 1.0, 6553.5}


# ------------------------------------------------------------------------------------------------ streamer content
def test_stream_content_tells_every_frame_apart_at_every_pixel():
    L, B, H, W = 25, 2, 6, 10
    d, c = ic.stream_content(L, B, H, W)
    assert d.dtype == np.uint16 and d.shape == (L, B, H, W) and c.dtype == np.uint8 and c.shape == (L, B, H, W, 3)
    fd, fc = d.reshape(L * B, H * W), c.reshape(L * B, H * W, 3)
    for p in range(H * W):
        assert len(set(fd[:, p].tolist())) == L * B and len(set(fc[:, p, 0].tolist())) == L * B
    assert (d >= 32768).any() and (d < 32768).any() and len(np.unique(c[0, 0])) > 16
    d2, c2 = ic.stream_content(L, B, H, W)
    assert np.array_equal(d, d2) and np.array_equal(c, c2)
