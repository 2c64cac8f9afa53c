"""GPU tests of the one half-iteration driver behind the single ICP solve (gs_icp_f32, gs_icp_dc_f32, gs_icp_map_dc_f32,
gs_icp_tape_f32) and the batched localisation (gs_localize_batch_f32).  The single solve is the B = 1 client of the
batched driver with every engine off: which state slot, which row buffer and which cloud a launch uses is written once,
so the two clients must agree bit for bit, and so must the solve with and without a tape, at the sizes where that
indexing can go wrong: around one row unit of FS_QPB = 96 source points, beyond FS_REDUCE_ROWS = 1024 rows (both
row-sum paths), and at 0 - 3 iterations (the degenerate result, each parity of the cloud ping-pong and of the final
state slot).  Every comparison is between entry points of the library under test, on a synthetic smooth surface."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def dev(a):
    return T(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def _surface(u, v, K):
    """camera-frame points and unit normals (towards the camera) of a smooth surface over pixel coordinates (u, v)"""
    f, cx, cy = K[0, 0], K[0, 2], K[1, 2]

    def point(u, v):
        z = 2.0 + 0.02 * u + 0.015 * v + 0.05 * np.sin(0.3 * u + 0.2) * np.cos(0.2 * v)
        return np.stack([(u - cx) / f * z, (v - cy) / f * z, z], -1)

    p = point(u, v)
    n = np.cross(point(u + 1e-3, v) - p, point(u, v + 1e-3) - p)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[n[..., 2] > 0] *= -1.0
    return p, n


@functools.lru_cache(maxsize=None)
def _scene(H, W):
    """A map of the surface in world coordinates (rows beyond the image border included: the target filter drops them)
    and a live frame of it, seen from a camera a centimetre and a few milliradians off the previous pose."""
    rng = np.random.default_rng(1000 * H + W)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 40.0
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    step = 0.5 if H * W < 1000 else 1.0
    mu, mv = np.meshgrid(np.arange(-2.0, W + 1.75, step) + 0.1, np.arange(-2.0, H + 1.75, step) + 0.1)
    P, N = _surface(mu.ravel(), mv.ravel(), K)
    prev = _rigid(0.02, -0.03, 0.01, [0.1, -0.05, 0.2])
    Pw, Nw = P @ prev[:3, :3].T + prev[:3, 3], N @ prev[:3, :3].T
    pu, pv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    V, _ = _surface(pu, pv, K)
    D = np.linalg.inv(_rigid(0.004, -0.003, 0.002, [0.006, -0.004, 0.008]))
    V = V @ D[:3, :3].T + D[:3, 3]
    depth = V[..., 2].copy()
    depth[rng.random(depth.shape) < 0.06] = 0.0   # holes: NaN rows of the lattice source
    return dict(K=dev(K), prev=dev(prev), P=dev(Pw), N=dev(Nw), vertex=dev(V), depth=dev(depth))


def _single(ops, s, H, W, mode, numiters):
    src = ops.lattice_source(s["vertex"], s["depth"], s["prev"], 1)
    assert src.shape[0] == H * W
    pix = ops.project_map(s["P"], s["prev"], s["K"], H, W)
    return ops.icp_map(src, s["P"], s["N"], pix, W, 1, compose=s["prev"], mode=mode, numiters=numiters)


def _batched(ops, s, mode, numiters):
    maps = [(s["P"], s["N"], s["P"].shape[0], None)]
    return ops.localize_batch(s["vertex"][None], s["depth"][None], s["K"][None], s["prev"][None], maps, 1, mode=mode,
                              numiters=numiters)[0]


# lattice counts 88 (below one row unit), 96 (exactly one), 97 (one over: a second row of one point)
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("H,W", [(8, 11), (8, 12), (97, 1)])
def test_single_solve_equals_batched_b1_around_one_row_unit(ops, H, W, mode):
    """gs_lattice_source_f32 + gs_project_map_f32 + gs_icp_map_dc_f32 == gs_localize_batch_f32 with B = 1, the 16 floats
    bit for bit (the comment above LocSeq promises it), for 0, 1, 2 and 3 iterations."""
    s = _scene(H, W)
    for numiters in (0, 1, 2, 3):
        one, bat = _single(ops, s, H, W, mode, numiters), _batched(ops, s, mode, numiters)
        assert torch.equal(bits(one), bits(bat)), (numiters, one, bat)
        if W > 1:   # (a one-pixel-wide image is a line of points: its solve is rank deficient, the bits still agree)
            assert bool(torch.isfinite(one).all()), (numiters, one)
            assert torch.equal(one, s["prev"]) == (numiters == 0), (numiters, one)   # (the first step moves the pose)
    # numiters 0: the composed initial transform, i.e. the previous pose itself
    assert torch.equal(_batched(ops, s, mode, 0), s["prev"])


@pytest.mark.parametrize("mode", [1, 0])
def test_single_solve_equals_batched_b1_beyond_reduce_rows(ops, mode):
    """320 x 320 at dsratio 1: 102 400 source points = 1067 rows > FS_REDUCE_ROWS, so every look-ahead and the finish
    read the one row the row-sum launch left; 2 iterations."""
    H = W = 320
    s = _scene(H, W)
    one, bat = _single(ops, s, H, W, mode, 2), _batched(ops, s, mode, 2)
    assert torch.equal(bits(one), bits(bat)), (one, bat)
    assert bool(torch.isfinite(one).all()) and not torch.equal(one, s["prev"])


def _clouds(n_src, n_tgt_side):
    """n_src source points a few millimetres off a surface sampled by n_tgt_side ** 2 targets"""
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 40.0
    K[0, 2] = K[1, 2] = 16.0
    rng = np.random.default_rng(n_src)
    tu, tv = np.meshgrid(np.linspace(0.0, 32.0, n_tgt_side), np.linspace(0.0, 32.0, n_tgt_side))
    tgt, tn = _surface(tu.ravel(), tv.ravel(), K)
    src, _ = _surface(rng.uniform(2.0, 30.0, n_src), rng.uniform(2.0, 30.0, n_src), K)
    D = _rigid(0.004, -0.003, 0.002, [0.006, -0.004, 0.008])
    return dev(src @ D[:3, :3].T + D[:3, 3]), dev(tgt), dev(tn)


# 97 points: one row unit and a second one of a single point.  gs_icp_tape_f32 takes no device-side counts and
# gs_knn_use_grid asks for 256 source points, so at 97 points NEITHER of the two ways onto the grid path is open to the
# tape entry point: that case runs the brute-force path on both sides.  The case of 257 source points (two row units and
# 65 points) against 2304 targets is above the threshold: it is the one that runs the shared driver, with the tape slots
# as its clouds.
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n_src,n_tgt_side", [(97, 12), (257, 48)])
def test_tape_solve_equals_plain_solve(ops, n_src, n_tgt_side, mode):
    """gs_icp_tape_f32 == gs_icp_f32 on the same inputs: T and idx bit for bit, and the trace stored in the tape is the
    trace of the plain solve; 3 iterations (both parities of the tape's index slots and a final state slot of each)."""
    src, tgt, tn = _clouds(n_src, n_tgt_side)
    K = 3
    T0, idx0, trace0 = ops.icp(src, tgt, tn, mode=mode, numiters=K, return_trace=True)
    T1, idx1, tape, _ = ops.icp_with_tape(src, tgt, tn, mode=mode, numiters=K)
    assert torch.equal(bits(T0), bits(T1)), (T0, T1)
    assert torch.equal(idx0, idx1)
    assert bool(torch.isfinite(T0).all()) and int(idx0.min()) >= 0
    trace1 = tape[: 4 * 12 * K].view(torch.float32).view(K, 12)   # (gs_icp_math.h: the trace is the tape's first region)
    assert torch.equal(bits(trace0), bits(trace1)), (trace0, trace1)


def test_device_side_counts_equal_exact_sizes_at_97_points(ops):
    """gs_icp_dc_f32 with the true counts on the device, on buffers with poisoned rows behind them (sources that would
    match and targets that would be matched if a kernel looked at them), == the exact-size call, bit for bit.  Device
    counts always take the grid path; the exact-size call of 97 points takes the brute-force path, so it is compared
    against the exact-size buffers WITH device counts as well (the same path on both sides)."""
    src, tgt, tn = _clouds(97, 12)
    n_s, n_t = src.shape[0], tgt.shape[0]
    srcb = torch.cat([src, tgt[:40] + 1e-4])
    tgtb = torch.cat([tgt, src[:50], torch.full((7, 3), 1e9, device="cuda")])
    tnb = torch.cat([tn, tn[:50], torch.full((7, 3), 7.0, device="cuda")])
    cnt = lambda n: torch.tensor([n], dtype=torch.int64, device="cuda")  # noqa: E731
    for mode in (1, 0):
        T_ref, idx_ref = ops.icp(src, tgt, tn, mode=mode, numiters=3)
        T_dc, idx_dc = ops.icp(src, tgt, tn, mode=mode, numiters=3, n_src_dev=cnt(n_s), n_tgt_dev=cnt(n_t))
        T, idx = ops.icp(srcb, tgtb, tnb, mode=mode, numiters=3, n_src_dev=cnt(n_s), n_tgt_dev=cnt(n_t))
        assert torch.equal(bits(T), bits(T_dc)) and torch.equal(idx[:n_s], idx_dc), (mode, T, T_dc)
        assert torch.equal(bits(T), bits(T_ref)) and torch.equal(idx[:n_s], idx_ref), (mode, T, T_ref)
        assert bool(torch.isfinite(T).all()) and int(idx[:n_s].max()) < n_t
