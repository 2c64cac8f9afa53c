"""Inputs shared by tests/test_ingest_cases_cpu.py (CPU) and tests/test_hip_ingest_stream.py (GPU).  No test lives here.

Three families, every one a deterministic function of its seed:

  * resize cases `(H0, W0) -> (H, W)` for gs_ingest_depth_u16_f32 / gs_ingest_color_u8_f32: sources with a side of 1 or 2,
    odd sources, one axis resized only (the depth kernel treats the axes separately, the colour kernel does not), integer
    and non-integer ratios both ways, a 1 x 1 target, and one target of more than one block;
  * native-conversion shapes `(n, H, W)` for gs_ingest_frames_native_f32, whose pixel counts sit on either side of one
    block and of one sweep of the capped grid, derived from the kernel's launch constants;
  * streamer content `(L, B, H, W)` in which every pixel of every `(t, b)` names its frame, so that a ring-slot mix-up
    changes bits.

Random pixel values, plus planted extremes (colour 0 / 255; depth 0, 1, 32767, 32768, 65535) at the four corners and
along the last row and column, where a resize that is one pixel off, a clamp that is one too wide or a signed read of
the depth shows.

The bound that the oracle's colour resize is held to against float64 is derived in `color_bound()`."""
import functools
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLOR_PLANT = (0, 255)
DEPTH_PLANT = (0, 1, 32767, 32768, 65535)

# ------------------------------------------------------------------------------------------------ resize
RESIZE_CASES = (
    # sources with a side of 1 or 2
    ((1, 1), (1, 1)), ((1, 1), (3, 5)),
    ((1, 7), (1, 7)), ((1, 7), (1, 1)), ((1, 7), (4, 14)), ((1, 7), (1, 3)),
    ((5, 1), (5, 1)), ((5, 1), (1, 1)), ((5, 1), (10, 3)), ((5, 1), (2, 1)),
    ((2, 3), (2, 3)), ((2, 3), (1, 1)), ((2, 3), (4, 6)), ((2, 3), (1, 3)), ((2, 3), (2, 1)),
    ((2, 3), (240, 320)),                                    # more than one block of 256 pixels in each kernel
    # an odd source: same size, 1 x 1, one axis only (up and down), non-integer ratios both ways, integer ratios
    ((23, 31), (23, 31)), ((23, 31), (1, 1)),
    ((23, 31), (23, 40)), ((23, 31), (9, 31)), ((23, 31), (40, 31)), ((23, 31), (23, 9)),
    ((23, 31), (37, 53)), ((23, 31), (10, 7)), ((23, 31), (46, 62)), ((23, 31), (69, 31)),
    # an even source: integer ratios down and up, mixed
    ((24, 32), (24, 32)), ((24, 32), (1, 1)), ((24, 32), (12, 16)), ((24, 32), (8, 8)), ((24, 32), (48, 96)),
    ((24, 32), (6, 64)), ((24, 32), (17, 45)),
)
RESIZE_SCALE_DIVS = (5000.0, 1000.0)


def resize_name(case):
    (h0, w0), (h, w) = case
    return "%dx%d_to_%dx%d" % (h0, w0, h, w)


def _plant(img, values):
    """values, cycling, along the last row and up the last column of img (H, W) or (H, W, C), and the largest at the first
    pixel: all four corners are planted, and neighbours on the last row / column always differ"""
    h, w = img.shape[:2]
    k = len(values)
    img[0, 0] = values[-1]
    for x in range(w):
        img[h - 1, x] = values[x % k]
    for y in range(h):
        img[y, w - 1] = values[(w - 1 + h - 1 - y) % k]
    return img


@functools.lru_cache(maxsize=None)
def resize_source(h0, w0, seed=811):
    """(depth uint16 (h0, w0), colour uint8 (h0, w0, 3)) of a source size, read-only"""
    rng = np.random.default_rng([seed, h0, w0])
    d = _plant(rng.integers(0, 65536, (h0, w0)).astype(np.uint16), DEPTH_PLANT)
    c = _plant(rng.integers(0, 256, (h0, w0, 3)).astype(np.uint8), COLOR_PLANT)
    d.setflags(write=False)
    c.setflags(write=False)
    return d, c


def planted_step(img):
    """smallest difference between neighbours along the planted last row and last column (inf where there are none):
    what a resize that is one source pixel off changes a border pixel by, at least"""
    a = np.asarray(img).astype(np.float64)
    a = a.reshape(a.shape[0], a.shape[1], -1)
    steps = [np.abs(np.diff(a[-1], axis=0)).ravel(), np.abs(np.diff(a[:, -1], axis=0)).ravel()]
    steps = np.concatenate(steps)
    return float(steps.min()) if steps.size else float("inf")


def _half_ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) / 2


def lin_coord_max(n_dst, n_src):
    """the largest source coordinate (d + 0.5) * n_src / n_dst - 0.5 of an axis"""
    return (n_dst - 0.5) * n_src / n_dst - 0.5


def color_bound(case, normalize=False):
    """How far oracle.ingest_color (OpenCV's arithmetic) may be from pixel-centre bilinear interpolation in float64.

    OpenCV rounds the source coordinate x = (d + 0.5) * scale - 0.5 to float32 BEFORE it takes the weights (f = x -
    floor(x), 1 - f) from it, and keeps the weights in float32; the sums are float64.  Along one axis the interpolant
    (1 - f) p0 + f p1, with the clamp at both borders, is a continuous, piecewise linear function of x whose slope is at
    most the value range R (255, or 1 after / 255), so moving x by e moves it by at most |e| R -- also where the rounding
    carries x across a source pixel or across a clamp.  |e| is at most half a float32 ulp at the largest coordinate of
    the axis.  (x - floor(x) is exact in float32; 1 - f rounds only where x < 1/2, by at most 2**-25, and there e is at
    most 2**-26: together below half an ulp at any largest coordinate of 1 or more.  An axis that keeps its size, and a
    source of one pixel, have integer coordinates or a clamped weight of 0: no error, the term is kept anyway.)  The
    second axis interpolates values that are again within the range R.  The cast to float32 adds half a float32 ulp of
    the result, which is at most R.

        bound = (half_ulp32(xmax) + half_ulp32(ymax)) * R + half_ulp32(R)

    The float64 roundings of either side (a few 2**-53 R) are five orders of magnitude below the smallest term."""
    (h0, w0), (h, w) = case
    R = 1.0 if normalize else 255.0
    return (_half_ulp32(lin_coord_max(w, w0)) + _half_ulp32(lin_coord_max(h, h0))) * R + _half_ulp32(R)


# the bound of every case, stated next to its derivation: name -> (normalize off, normalize on)
COLOR_BOUNDS = {resize_name(c): (color_bound(c, False), color_bound(c, True)) for c in RESIZE_CASES}


# ------------------------------------------------------------------------------------------------ native conversion
def kernel_constants():
    """(threads per block, GS_INGEST_BLOCKS, pixels per work item) of gs_ingest_native4_kernel, read from its source"""
    src = open(os.path.join(REPO, "gradslam_amd", "csrc", "gs_ingest.hip")).read()
    blocks = int(re.search(r"constexpr\s+int\s+GS_INGEST_BLOCKS\s*=\s*(\d+)\s*;", src).group(1))
    threads = int(re.search(r"__launch_bounds__\((\d+)\)\s+gs_ingest_native4_kernel", src).group(1))
    assert re.search(r"\+=\s*\(int64_t\)gridDim\.x \* %d\b" % threads, src), "the grid-stride step is not blocks x threads"
    assert "px / 4" in src and "reinterpret_cast<const uint2*>(depth_raw)" in src      # 4 pixels per item
    return threads, blocks, 4


THREADS, BLOCKS, PX_PER_ITEM = kernel_constants()
SWEEP = THREADS * BLOCKS            # work items that one sweep of the capped grid serves
# Work items of a launch over px pixels (n_quads = px / 4): both modalities n_quads + 3 n_quads = px, colour only
# 3 n_quads, depth only n_quads.
_Q_COLOR = SWEEP // 3               # colour only: 3 q never equals a sweep of 2**15 items; q, q + 1 are its two sides


def native_pixel_counts():
    one_block = [PX_PER_ITEM, THREADS - PX_PER_ITEM, THREADS, THREADS + PX_PER_ITEM]            # 4, 252, 256, 260
    both = [SWEEP - PX_PER_ITEM, SWEEP, SWEEP + PX_PER_ITEM]                                     # items = px
    color = [PX_PER_ITEM * q for q in (_Q_COLOR - 1, _Q_COLOR, _Q_COLOR + 1)]                    # items = 3 px / 4: one sweep short by 5, by 2, over by 1
    depth = [PX_PER_ITEM * q for q in (SWEEP - 1, SWEEP, SWEEP + 1)]                             # items = px / 4
    many = [3 * SWEEP + 5 * THREADS + PX_PER_ITEM,            # > 3 sweeps with both, > 2 colour only, ragged last sweep
            PX_PER_ITEM * (2 * SWEEP + THREADS + 1)]          # > 2 sweeps depth only
    return one_block + both + color + depth + many


def _shape_of(px):
    """(n, H, W) with n * H * W = px; where px / 4 is odd the frames themselves are no multiple of 4 pixels"""
    q = px // PX_PER_ITEM
    if q % 2 == 1 and q > 1:
        return (4, 1, q)
    for h in (16, 12, 8, 6, 4, 2, 1):
        if px % h == 0:
            return (1, h, px // h)


NATIVE_SHAPES = tuple([_shape_of(px) for px in native_pixel_counts()] + [(4, 3, 5), (2, 5, 6)])
NATIVE_SCALE_DIVS = (5000.0, 1000.0, 1.0, 6553.5)
NATIVE_MODES = ("both", "depth", "color")
assert all(n * h * w % PX_PER_ITEM == 0 for n, h, w in NATIVE_SHAPES)
assert any(n > 1 and h * w % PX_PER_ITEM for n, h, w in NATIVE_SHAPES)


def native_name(shape):
    return "%dx%dx%d" % shape


@functools.lru_cache(maxsize=None)
def native_raw(shape, seed=822):
    """(depth uint16 (n, H, W), colour uint8 (n, H, W, 3)) read-only: random, every planted value in every position of
    the first and of the last work item (both halves of both words of a depth quad, every byte of a colour word)"""
    n, h, w = shape
    px = n * h * w
    rng = np.random.default_rng([seed, px])
    d = rng.integers(0, 65536, px).astype(np.uint16)
    c = rng.integers(0, 256, 3 * px).astype(np.uint8)
    for i in range(min(px, 20)):
        d[i] = DEPTH_PLANT[(i % 4 + i // 4) % len(DEPTH_PLANT)]
        d[px - 1 - i] = DEPTH_PLANT[(i % 4 + i // 4 + 3) % len(DEPTH_PLANT)]
    for i in range(min(3 * px, 16)):
        c[i] = COLOR_PLANT[(i % 4 + i // 4) % 2]
        c[3 * px - 1 - i] = COLOR_PLANT[(i % 4 + i // 4 + 1) % 2]
    d, c = d.reshape(n, h, w), c.reshape(n, h, w, 3)
    d.setflags(write=False)
    c.setflags(write=False)
    return d, c


def native_depth_ref(raw_u16, scale_div):
    """the float64 statement of the conversion, cast last"""
    return (np.asarray(raw_u16).astype(np.float64) / np.float64(scale_div)).astype(np.float32)


def native_color_ref(raw_u8, normalize):
    v = np.asarray(raw_u8).astype(np.float64)
    return (v / 255.0 if normalize else v).astype(np.float32)


# ------------------------------------------------------------------------------------------------ streamer content
def stream_content(L, B, H, W):
    """(depth uint16 (L, B, H, W), colour uint8 (L, B, H, W, 3)), pure functions of (t, b, y, x): every pixel of the depth
    and the first colour channel of every pixel hold t * B + b (modulo a prime above it), so that no two (t, b) agree
    anywhere; the other bits mix in the position"""
    assert L * B < 251
    t, b, y, x = np.meshgrid(np.arange(L), np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    f = t * B + b                                                   # the frame's number, < 251
    d = (f * 257 + ((y * 31 + x * 7) % 257)) % 65536                # f * 257 + r with r < 257: f is recoverable
    d[:, :, 0, 0] = np.where(f[:, :, 0, 0] % 2 == 0, 65535 - f[:, :, 0, 0], 32768 + f[:, :, 0, 0])   # >= 32768, still one per frame
    c = np.stack([f, (f * 3 + y * 5 + x) % 256, (255 - f + y + x * 11) % 256], -1)
    return np.ascontiguousarray(d.astype(np.uint16)), np.ascontiguousarray(c.astype(np.uint8))
