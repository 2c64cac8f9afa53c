"""GPU tests of the free-space carve (gs_carve.hip -> gs_free_space_dc_f32 -> ops.free_space_batch ->
Pointclouds.carve_ -> PointFusion(carve_margin=...)) against its NumPy restatement (tests/carve_ref.py) and, end to
end, against the oracle frame loop that applies the restatement between the frames.

The outputs of the pass are integers and the removal moves bits, so every comparison is for EQUALITY: no tolerance
anywhere.  Block = 256 rows, 16 cameras per LDS group, 8 sequences per launch: the sizes sit on and around those."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import slam as oslam
from tests import carve_ref as cr
from tests import prune_ref as pr
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
f32 = np.float32
NAN = float("nan")
H, W, LMAX, NROWS = 37, 53, 17, 1027
FX, CX, CY = 45.0, 26.0, 18.0
K = np.array([[FX, 0, CX, 0], [0, FX, CY, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
EXACT = 0.0625                 # a margin that float32 holds exactly: 1.0625 - 1.0 == 0.0625
SENT32, SENT8 = -77, 0xAB      # values the pass never writes: an element left alone keeps them


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gs():
    assert torch.cuda.is_available()
    import gradslam_amd
    return gradslam_amd


def at(h, w, z):
    """the point of depth z on the ray through the centre of pixel (h, w) of view 0 (the identity pose)"""
    return [(w - CX) * z / FX, (h - CY) * z / FX, z]


# pixels of view 0 the special rows sit on
BORDER = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 25), (H - 1, 25), (8, 0), (8, W - 1)]
PX_ALL, PX_EQ, PX_ULP, PX_CORNER, PX_HOLE = (18, 26), (5, 5), (5, 12), (30, 8), (30, 20)
PX_ZERO, PX_NEG, PX_NAN = (30, 30), (30, 36), (30, 42)
SPECIAL = [PX_ALL, PX_EQ, PX_ULP, PX_CORNER, PX_HOLE, PX_ZERO, PX_NEG, PX_NAN] + BORDER
N_SPECIAL = len(SPECIAL) + 4


def _build():
    rng = np.random.default_rng(2024)
    poses = np.tile(np.eye(4, dtype=f32), (LMAX, 1, 1))
    for l in range(1, LMAX):
        a = rng.uniform(-0.02, 0.02)
        poses[l, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], f32)
        poses[l, :3, 3] = rng.uniform(-0.03, 0.03, 3).astype(f32)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depths = np.empty((LMAX, H, W), f32)
    for l in range(LMAX):
        d = (2.0 + 0.3 * np.sin(0.2 * hh + 0.1 * l) * np.cos(0.15 * ww)).astype(f32)
        h0, w0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
        d[h0:h0 + 8, w0:w0 + 8] = 1.0                      # something near: a depth edge on four sides
        r = rng.random((H, W))
        d[r < 0.06] = 0.0
        d[(r >= 0.06) & (r < 0.07)] = -1.5
        d[(r >= 0.07) & (r < 0.08)] = NAN
        d[10:27, 18:35] = 1.75                              # the middle of every view is measured, and far
        depths[l] = d
    D0 = depths[0]
    for h, w in SPECIAL[1:]:
        D0[max(h - 3, 0):h + 4, max(w - 3, 0):w + 4] = 2.0
    D0[3:8, 3:8] = f32(1.0) + f32(EXACT)
    D0[3:8, 10:15] = np.nextafter(f32(1.0) + f32(EXACT), f32(9))
    D0[31, 9] = 1.0                                         # the only pixel of the window that does not violate: a corner
    D0[29, 19], D0[31, 21] = 0.0, NAN                       # holes in a window that otherwise violates
    D0[PX_ZERO], D0[PX_NEG], D0[PX_NAN] = 0.0, -2.0, NAN
    special = [at(18, 26, 0.4)] + [at(h, w, 1.0) for h, w in SPECIAL[1:]] + \
        [[0, 0, -1.0], [0.1, 0.1, -0.5], [5, 0, 1.0], [0, -5, 1.0]]       # behind the camera, outside the frame
    pts = [np.array(special, f32)]
    # rows hung on the depth images: a pixel of some view, at an offset from the depth it shows
    n = NROWS - N_SPECIAL - 100
    v = rng.integers(0, LMAX, n)
    ph = np.where(rng.random(n) < 0.2, rng.choice([0, H - 1], n), rng.integers(0, H, n))
    pw = np.where(rng.random(n) < 0.2, rng.choice([0, W - 1], n), rng.integers(0, W, n))
    d = depths[v, ph, pw]
    z = np.where(d > 0, d, 2.0) + rng.choice([-0.6, -0.2, -0.051, -0.049, 0.0, 0.02, 0.4], n)
    cam = np.stack([(pw + rng.uniform(-0.45, 0.45, n) - CX) * z / FX, (ph + rng.uniform(-0.45, 0.45, n) - CY) * z / FX, z], 1)
    pts.append((np.einsum("nij,nj->ni", poses[v, :3, :3].astype(np.float64), cam) + poses[v, :3, 3]).astype(f32))
    # and rows anywhere, also behind and beside the cameras
    pts.append(np.stack([rng.uniform(-2, 2, 100), rng.uniform(-2, 2, 100), rng.uniform(-1, 3, 100)], 1).astype(f32))
    P = np.concatenate(pts)
    assert P.shape == (NROWS, 3)
    return P, depths, poses


_FIX = {}


def fixture_data():
    """(points (1027, 3), depths (17, 37, 53), poses (17, 4, 4)); computed once and never changed"""
    if "d" not in _FIX:
        _FIX["d"] = _build()
    return _FIX["d"]


_REF = {}


def ref(n, L, margin, window, min_views=1, n_bound=None):
    """the restatement on the first n rows and the first L views (cached: the references are shared and left alone)"""
    key = (n, L, margin, window, min_views, n_bound)
    if key not in _REF:
        P, D, Ts = fixture_data()
        _REF[key] = cr.free_space(P[:n if n_bound is None else n_bound], n, D[:L], Ts[:L], K, margin, window, min_views)
    return _REF[key]


def run(ops, P, n_dev, D, Ts, **kw):
    """ops.free_space into sentinel-filled outputs: every element must have been written"""
    rows = P.shape[0]
    out = (torch.full((rows,), SENT32, dtype=torch.int32, device="cuda"),
           torch.full((rows,), SENT8, dtype=torch.uint8, device="cuda"))
    r = ops.free_space(dev(P), dev(D), dev(Ts), dev(K), n_dev=n_dev, out=out, **kw)
    assert r.violations is out[0] and r.keep is out[1]
    return host(r.violations), host(r.keep)


# ------------------------------------------------------------------------------------------ kernel == restatement
@pytest.mark.parametrize("n", [1, 255, 256, 257, NROWS])
def test_kernel_equals_restatement(ops, n):
    P, D, Ts = fixture_data()
    for L in (1, 3, LMAX):                  # 17: more views than one LDS group of 16 cameras
        for window in (0, 1, 2):
            viol, keep = run(ops, P[:n], None, D[:L], Ts[:L], margin=0.05, window=window)
            want = ref(n, L, 0.05, window)
            assert viol.dtype == np.int32 and keep.dtype == np.uint8
            assert np.array_equal(viol, want[0]), (L, window, np.nonzero(viol != want[0])[0][:10])
            assert np.array_equal(keep, want[1]), (L, window)


def test_the_fixture_holds_every_case_and_the_kernel_gets_them_right(ops):
    P, D, Ts = fixture_data()
    L = LMAX
    pix0, z0 = cr.project(P, Ts[0], K, H, W)
    D0 = D[0]
    flat = lambda hw: hw[0] * W + hw[1]                                    # noqa: E731
    # --- what the fixture contains, from the restatement's pieces alone
    every = [cr.project(P, Ts[l], K, H, W) for l in range(L)]
    assert any(((p < 0) & ~(z > 0)).any() for p, z in every), "rows behind a camera"
    assert any(((p < 0) & (z > 0)).any() for p, z in every), "rows in front of a camera but outside its frame"
    s = {name: i for i, name in enumerate(["all", "eq", "ulp", "corner", "hole", "zero", "neg", "nan"])}
    for name, hw in zip(s, SPECIAL[:8]):
        assert pix0[s[name]] == flat(hw), name
    assert z0[s["eq"]] == f32(1.0) and f32(D0[PX_EQ] - z0[s["eq"]]) == f32(EXACT), "a row exactly at d - z == margin"
    assert f32(D0[PX_ULP] - z0[s["ulp"]]) > f32(EXACT)
    assert D0[PX_ZERO] == 0 and D0[PX_NEG] < 0 and np.isnan(D0[PX_NAN])
    for i, hw in enumerate(BORDER):
        assert pix0[8 + i] == flat(hw), ("border row", hw)
    one = lambda i, m, w: bool(cr.violates(P[i:i + 1], D0, Ts[0], K, m, w)[0])   # noqa: E731
    assert not one(s["eq"], EXACT, 0) and not one(s["eq"], EXACT, 2) and one(s["ulp"], EXACT, 0) and one(s["ulp"], EXACT, 2)
    assert one(s["corner"], 0.05, 0) and not one(s["corner"], 0.05, 1), "a window whose only veto is a corner"
    patched = D0.copy()
    patched[31, 9] = 2.0
    assert bool(cr.violates(P[s["corner"]:s["corner"] + 1], patched, Ts[0], K, 0.05, 1)[0]), "... and only that corner"
    assert all(one(s["hole"], 0.05, w) for w in (0, 1, 2)), "a window with holes still violates"
    assert not any(one(s[k], 0.05, w) for k in ("zero", "neg", "nan") for w in (0, 1, 2)), "a centre without depth"
    assert all(one(8 + i, 0.05, w) for i in range(len(BORDER)) for w in (0, 1, 2, 3)), "clipped windows on every border"
    for window in (0, 1, 2):
        v = ref(NROWS, L, 0.05, window)[0]
        assert v[s["all"]] == L and (v == 0).any() and (v == 1).any(), "rows violating 0, 1, all views"
    # --- and the kernel on all of it
    for margin in (0.05, EXACT, 0.0):
        for window in (0, 1, 2, 3):
            for min_views in (1, 2, L):
                viol, keep = run(ops, P, None, D, Ts, margin=margin, window=window, min_views=min_views)
                want = ref(NROWS, L, margin, window, min_views)
                assert np.array_equal(viol, want[0]), (margin, window, np.nonzero(viol != want[0])[0][:10])
                assert np.array_equal(keep, want[1]), (margin, window, min_views)
    assert len({ref(NROWS, L, 0.05, 1, mv)[1].tobytes() for mv in (1, 2, L)}) == 3     # min_views matters here


def test_rows_beyond_the_device_count_are_cleared_and_never_read(ops):
    P, D, Ts = fixture_data()
    n = 700
    Q = P.copy()
    Q[n:] = NAN
    n_dev = torch.tensor([n], dtype=torch.int64, device="cuda")
    viol, keep = run(ops, Q, n_dev, D[:3], Ts[:3], window=1)
    want = ref(n, 3, 0.05, 1, 1, NROWS)
    assert np.array_equal(viol, want[0]) and np.array_equal(keep, want[1])
    assert (viol[n:] == 0).all() and (keep[n:] == 0).all() and keep[:n].any() and (keep[:n] == 0).any()
    # rows that would violate if they were read: still 0 and 0
    viol2, keep2 = run(ops, P, n_dev, D[:3], Ts[:3], window=1)
    assert np.array_equal(viol2, viol) and np.array_equal(keep2, keep) and ref(NROWS, 3, 0.05, 1)[0][n:].any()
    # a device count above the bound is clamped to the bound
    big = torch.tensor([NROWS + 50], dtype=torch.int64, device="cuda")
    viol3, _ = run(ops, P, big, D[:3], Ts[:3], window=1)
    assert np.array_equal(viol3, ref(NROWS, 3, 0.05, 1)[0])


@pytest.mark.parametrize("counts", [(257,), (NROWS, 0, 300), (5, 1024, 257, 0, NROWS, 1, 513, 64, 1000)])
def test_batch_equals_single_calls(ops, counts):
    """B = 1, B = 3 in one launch group and B = 9 in two: every sequence as in a call of its own, and as the restatement;
    ragged counts, some of them on the device below their bound"""
    P, D, Ts = fixture_data()
    B, L = len(counts), 3
    maps, dd, tt, kk, singles = [], [], [], [], []
    for b, n in enumerate(counts):
        Pb = np.roll(P, -37 * b, axis=0)[:n + (b % 2) * 9]             # odd sequences: 9 rows beyond the device count
        views = [(5 * b + l) % LMAX for l in range(L)]
        Kb = K.copy()
        Kb[0, 2] += b                                                  # every sequence has its own intrinsics
        n_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if b % 2 else None
        maps.append((dev(Pb), None, None, None, None, n_dev))
        dd.append(D[views]); tt.append(Ts[views]); kk.append(Kb)
        want = cr.free_space(Pb, n, D[views], Ts[views], Kb, 0.05, 1, 2)
        one = ops.free_space(maps[b][0], dev(D[views]), dev(Ts[views]), dev(Kb), n_dev=n_dev, min_views=2)
        assert np.array_equal(host(one.violations), want[0]) and np.array_equal(host(one.keep), want[1]), b
        singles.append(want)
    got = ops.free_space_batch(maps, dev(np.stack(dd))[..., None], dev(np.stack(tt)), dev(np.stack(kk)), min_views=2)
    assert len(got.violations) == B and len(got.keep) == B
    for b, want in enumerate(singles):
        assert got.violations[b].dtype == torch.int32 and got.keep[b].dtype == torch.uint8
        assert np.array_equal(host(got.violations[b]), want[0]) and np.array_equal(host(got.keep[b]), want[1]), b


def test_either_output_may_be_left_out_and_strided_depth_is_read_in_place(ops):
    P, D, Ts = fixture_data()
    want = ref(NROWS, 3, 0.05, 1)
    Pd, Dd, Td, Kd = dev(P), dev(D[:3]), dev(Ts[:3]), dev(K)
    v = torch.full((NROWS,), SENT32, dtype=torch.int32, device="cuda")
    k = torch.full((NROWS,), SENT8, dtype=torch.uint8, device="cuda")
    r = ops.free_space(Pd, Dd, Td, Kd, out=(v, None))
    assert r.keep is None and np.array_equal(host(v), want[0]) and bool((k == SENT8).all())
    r = ops.free_space(Pd, Dd, Td, Kd, out=(None, k))
    assert r.violations is None and np.array_equal(host(k), want[1])
    with pytest.raises(ValueError, match="out"):
        ops.free_space(Pd, Dd, Td, Kd, out=(None, None))
    with pytest.raises(ValueError, match="out"):
        ops.free_space(Pd, Dd, Td, Kd, out=(v[:5], None))
    # every other view of a longer stack: a view, no copy (the stride between the views is passed on)
    stack = dev(D[:6])
    r = ops.free_space(Pd, stack[::2], dev(Ts[:6:2]), Kd)
    w = cr.free_space(P, NROWS, D[:6:2], Ts[:6:2], K, 0.05, 1, 1)
    assert np.array_equal(host(r.violations), w[0]) and np.array_equal(host(r.keep), w[1])
    # nothing is on the tape
    Pg = Pd.clone().requires_grad_(True)
    r = ops.free_space(Pg, Dd, Td, Kd)
    assert not r.violations.requires_grad and np.array_equal(host(r.violations), want[0])


# ------------------------------------------------------------------------------------------ Pointclouds
def device_map(gs, counts, extra=300):
    """a Pointclouds whose counts live on the device (one group), on buffers with `extra` rows of room that hold NaN
    points; rows of the fixture, other attributes of random bits"""
    P, _, _ = fixture_data()
    B = len(counts)
    pc = gs.Pointclouds(device="cuda")
    pc._init_empty_batch(B, 1)
    arrs = []
    for b, n in enumerate(counts):
        rng = np.random.default_rng(50 + b)
        Pb = np.concatenate([np.roll(P, -11 * b, axis=0)[:n], np.full((extra, 3), NAN, f32)])
        raw = lambda c: rng.integers(0, 1 << 32, size=(n + extra, c), dtype=np.uint64).astype(np.uint32).view(f32)  # noqa: E731
        arrs.append((Pb, raw(3), raw(3), rng.random((n + extra, 1), dtype=f32)))
        for k, a in zip(("points", "normals", "colors", "features"), arrs[-1]):
            pc._buf[k][b] = dev(a)
    cnt = torch.tensor(counts, dtype=torch.int64, device="cuda")
    pc._n_host[:] = list(counts)
    pc._set_counts_dev(cnt, 0)
    pc._set_counts_dev(cnt, extra)
    torch.cuda.synchronize()
    pc._dcount[0].group.poll()
    assert pc._dcount[0].group.bounds == [n + extra for n in counts] and not pc._dcount[0].group._pending
    return pc, arrs


def frames_for(gs, B, L):
    _, D, Ts = fixture_data()
    views = [[(3 * b + l) % LMAX for l in range(L)] for b in range(B)]
    d = np.stack([D[v] for v in views])[..., None]
    return gs.RGBDImages(torch.zeros(B, L, H, W, 3, device="cuda"), dev(d), dev(np.tile(K, (B, 1, 1, 1))),
                         dev(np.stack([Ts[v] for v in views]))), views


def test_pointclouds_carve_equals_the_restated_prune_and_keeps_the_counts_on_the_device(gs):
    _, D, Ts = fixture_data()
    counts = (NROWS, 300)
    pc, arrs = device_map(gs, counts)
    frames, views = frames_for(gs, 2, 3)
    viol = pc.free_space_violations(frames, margin=0.05, window=1)
    assert len(pc._dcount) == 2, "reading the violations resolved a device-side count"
    pc.mark_epoch()
    marks0 = host(pc._marks[:, 0]).tolist()
    assert marks0 == list(counts)
    pc._marks[:, 0] //= 2                       # an older epoch, somewhere inside the maps
    bounds = list(pc._dcount[0].group.bounds)
    caps = [t.shape[0] for t in pc._buf["points"]]
    gen = pc._generation
    assert pc.carve_(frames, margin=0.05, window=1, min_views=2) is pc
    assert len(pc._dcount) == 2, "the carve resolved a device-side count"
    assert pc._dcount[0].group.bounds == bounds, "the bounds change only when a read-back lands"
    assert [t.shape[0] for t in pc._buf["points"]] == caps and pc._generation > gen
    assert pc.last_pruned.is_cuda
    want = []
    for b, n in enumerate(counts):
        v, keep = cr.free_space(arrs[b][0], n, D[views[b]], Ts[views[b]], K, 0.05, 1, 2)
        assert viol[b].dtype == torch.int32 and np.array_equal(host(viol[b]), v), b
        want.append(pr.prune(*arrs[b], n, None, keep, [n // 2], -1))
        assert 0 < want[-1][5] < n
    assert pc._tighten_counts() == [w[4] for w in want]
    assert host(pc.last_pruned).tolist() == [w[5] for w in want]
    assert host(pc._marks[:, 0]).tolist() == [w[6][0] for w in want], "the marks are rewritten"
    for b, w in enumerate(want):
        for k, a in zip(("points", "normals", "colors", "features"), w[:4]):
            assert np.array_equal(bits(host(pc._buf[k][b][:w[4]])), bits(a)), (b, k)
    # out of place: the original stays
    out = pc.carve(frames, margin=0.0, window=0)
    assert out is not pc and pc._tighten_counts() == [w[4] for w in want] and sum(out._n) < sum(w[4] for w in want)


def test_carve_of_a_taped_map_keeps_the_rows_on_the_tape(gs):
    P, D, Ts = fixture_data()
    n = 300
    Pg = dev(P[:n]).requires_grad_(True)
    z = lambda c: dev(np.zeros((n, c), f32))   # noqa: E731
    pc = gs.Pointclouds([Pg], [z(3)], [z(3)], [z(1)])
    frames, views = frames_for(gs, 1, 3)
    out = pc.carve(frames)
    keep = cr.free_space(P[:n], n, D[views[0]], Ts[views[0]], K)[1] != 0
    assert out._n == [int(keep.sum())] and 0 < keep.sum() < n
    out.points_list[0].sum().backward()
    assert np.array_equal(host(Pg.grad), np.repeat(keep[:, None], 3, 1).astype(f32))


def test_backward_of_a_render_taken_before_a_carve_raises(gs):
    pc, _ = device_map(gs, (NROWS,), extra=0)
    frames, _ = frames_for(gs, 1, 1)
    pose = torch.eye(4, device="cuda").view(1, 1, 4, 4).clone().requires_grad_(True)
    stale = pc.render(dev(K).view(1, 1, 4, 4), pose, H, W, differentiable=True).depth_image.sum()
    pc.carve_(frames)
    with pytest.raises(RuntimeError, match="changed in place"):
        stale.backward()


# ------------------------------------------------------------------------------------------ end to end
L_SEQ = cr.SEQ_L
CARVE = dict(carve_margin=0.05, carve_window=1)
PRUNE = dict(prune_min_confidence=0.004, prune_min_age=2, prune_every=2)
FILTER = dict(radius=2, sigma_space=1.5, sigma_range=0.05)


def oracle_run(s, depths, prune=False, marks=None):
    """the oracle loop (gradICP odometry) with the restated carve after every step's map update -- a prune by the restated
    keep mask, which also rewrites the epoch marks -- and, with `prune`, the restated pruning schedule after it; `marks`:
    a list that receives the epoch marks"""
    Kc = s["intrinsics"][0]
    marks, removed = [] if marks is None else marks, []

    def per_frame(i, m, pose):
        n = len(m)
        _, keep = cr.free_space(m.points, n, [depths[i]], [pose], Kc, 0.05, 1, 1)
        out = pr.prune(m.points, m.normals, m.colors, m.ccounts, n, None, keep, marks, -1)
        removed.append(out[5])
        m.points, m.normals, m.colors, m.ccounts = out[:4]
        marks[:] = out[6]
        if not prune:
            return
        if (i + 1) % PRUNE["prune_every"] == 0 and len(marks) >= PRUNE["prune_min_age"]:
            out = pr.prune(m.points, m.normals, m.colors, m.ccounts, len(m), PRUNE["prune_min_confidence"], None, marks,
                           len(marks) - PRUNE["prune_min_age"])
            m.points, m.normals, m.colors, m.ccounts = out[:4]
            marks[:] = out[6]
        marks.append(len(m))

    m, poses = oslam.run_sequence(s["colors"], depths, Kc, s["poses"], odom="gradicp", per_frame=per_frame)
    return m, poses, removed


def frames_of(gs, s, depths):
    poses = T(s["poses"][None]).cuda()
    poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(np.ascontiguousarray(depths)[None]).cuda(),
                         T(s["intrinsics"][None]).cuda(), poses)


def step_loop(gs, slam, frames, inplace=True):
    pc, prev, rec, removed = gs.Pointclouds(device="cuda"), None, [], []
    for i in range(L_SEQ):
        live = frames[:, i]
        pc, p = slam.step(pc, live, prev, inplace=inplace)
        prev = live
        rec.append(host(p[0, 0]))
        removed.append(pc.last_pruned)
    return pc, np.stack(rec), removed


def same_as_oracle(pc, poses, m, oposes, what):
    got = [host(x[0]) for x in (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)]
    assert got[0].shape == m.points.shape, (what, got[0].shape, m.points.shape)
    for name, a, b in zip(("points", "normals", "colors", "ccounts", "poses"), got + [poses],
                          (m.points, m.normals, m.colors, m.ccounts, oposes)):
        assert np.array_equal(bits(a), bits(b)), "%s %s: %d of %d differ" % (what, name, (a != b).sum(), a.size)


@pytest.fixture(scope="module")
def moved():
    s = cr.block_sequence("wave", moved=True)
    m, poses, removed = oracle_run(s, s["depths"])
    plain, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gradicp")
    print("oracle carve, rows removed per step:", removed, "final", len(m), "uncarved", len(plain))
    assert sum(removed) > 600 and len(m) < len(plain)
    return s, m, poses, removed, plain


@pytest.fixture(scope="module")
def stepped(gs, moved):
    """the moved-block sequence stepped in place with the carving PointFusion (fast path from the third frame on)"""
    s = moved[0]
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE)
    pc, poses, removed = step_loop(gs, slam, frames_of(gs, s, s["depths"]))
    assert getattr(slam, "_step_plan", None) is not None, "the in-place loop must have taken the fast path"
    assert len(pc._dcount) == 1, "the counts stay on the device through the carves"
    return pc, poses, removed


def test_carving_slam_equals_the_carving_oracle(moved, stepped):
    s, m, oposes, oremoved, _ = moved
    pc, poses, removed = stepped
    assert [int(r[0]) for r in removed] == oremoved
    assert pc._carve_steps == L_SEQ
    same_as_oracle(pc, poses, m, oposes, "fast path")


def test_undisturbed_sequence_loses_no_row_and_equals_the_plain_run(gs):
    s = cr.block_sequence("wave", moved=False)
    m, oposes, oremoved = oracle_run(s, s["depths"])
    assert oremoved == [0] * L_SEQ
    pc, poses, removed = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE), frames_of(gs, s, s["depths"]))
    assert [int(r[0]) for r in removed] == [0] * L_SEQ
    same_as_oracle(pc, poses, m, oposes, "undisturbed")
    plain, pposes, _ = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda"), frames_of(gs, s, s["depths"]))
    same_as_oracle(plain, pposes, m, oposes, "carve_margin=None")


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from tests import carve_ref as cr
s = cr.block_sequence("wave", moved=True)
T = torch.from_numpy
poses = T(s["poses"][None]).cuda(); poses[:, 1:] = poses[:, :1]
frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
slam = gs.slam.PointFusion(odom="gradicp", device="cuda", carve_margin=0.05, carve_window=1)
pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
for i in range(cr.SEQ_L):
    live = frames[:, i]
    pc, p = slam.step(pc, live, prev, inplace=True)
    prev = live
    rec.append(p[0, 0].cpu().numpy())
assert getattr(slam, "_step_plan", None) is None, "GRADSLAM_HIP_FASTPATH=0 must keep the fast path out"
np.savez(sys.argv[1], poses=np.stack(rec), pts=pc.points_list[0].cpu().numpy(), nrm=pc.normals_list[0].cpu().numpy(),
         col=pc.colors_list[0].cpu().numpy(), cc=pc.features_list[0].cpu().numpy())
"""


def test_generic_path_carves_the_same(moved, tmp_path):
    s, m, oposes, _, _ = moved
    out = str(tmp_path / "generic.npz")
    subprocess.run([sys.executable, "-c", _CHILD % REPO, out], check=True, timeout=600,
                   env=dict(os.environ, GRADSLAM_HIP_FASTPATH="0"))
    z = np.load(out)
    for name, a, b in (("points", z["pts"], m.points), ("normals", z["nrm"], m.normals), ("colors", z["col"], m.colors),
                       ("ccounts", z["cc"], m.ccounts), ("poses", z["poses"], oposes)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), "generic path " + name


def test_forward_carves_the_same(gs, moved):
    s, m, oposes, _, _ = moved
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE)
    pc, poses = slam(frames_of(gs, s, s["depths"]))
    same_as_oracle(pc, host(poses[0]), m, oposes, "forward")


def test_carving_with_the_depth_filter_tests_what_was_fused(gs, moved):
    s = moved[0]
    raw = frames_of(gs, s, s["depths"])
    filtered = host(raw.bilateral_filter(**FILTER).depth_image[0])      # (pinned to its restatement by its own tests)
    assert not np.array_equal(bits(filtered), bits(s["depths"]))
    m, oposes, oremoved = oracle_run(s, filtered)
    assert sum(oremoved) > 600
    pc, poses, removed = step_loop(gs, gs.slam.PointFusion(odom="gradicp", device="cuda", depth_filter=FILTER, **CARVE), raw)
    assert [int(r[0]) for r in removed] == oremoved
    same_as_oracle(pc, poses, m, oposes, "depth_filter")


@pytest.fixture(scope="module")
def carved_and_pruned(moved):
    s, marks = moved[0], []
    m, oposes, oremoved = oracle_run(s, s["depths"], prune=True, marks=marks)
    assert sum(oremoved) > 600 and len(m) < len(moved[1])
    assert len(marks) == L_SEQ and marks[-1] == len(m)
    assert sum(oremoved[PRUNE["prune_min_age"]:]) > 600   # (carves rewrite marks that later prunes read)
    return m, oposes, marks


def test_carving_with_the_prune_schedule(gs, moved, carved_and_pruned):
    s = moved[0]
    m, oposes, marks = carved_and_pruned
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE, **PRUNE)
    pc, poses, _ = step_loop(gs, slam, frames_of(gs, s, s["depths"]))
    assert len(pc._dcount) == 1 and pc._prune_steps == L_SEQ and pc._carve_steps == L_SEQ
    assert host(pc._marks[0, :pc._n_marks]).tolist() == marks
    same_as_oracle(pc, poses, m, oposes, "carve + prune")


def test_out_of_place_steps_carve_and_prune_the_same(gs, moved, carved_and_pruned):
    """inplace=False: every step returns a new container, which takes the marks and the step counters before the carve
    rewrites them; the map given to a step keeps its rows and its marks"""
    s = moved[0]
    m, oposes, marks = carved_and_pruned
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE, **PRUNE)
    pc, poses, _ = step_loop(gs, slam, frames_of(gs, s, s["depths"]), inplace=False)
    assert pc._prune_steps == L_SEQ and pc._carve_steps == L_SEQ
    assert host(pc._marks[0, :pc._n_marks]).tolist() == marks
    same_as_oracle(pc, poses, m, oposes, "out of place, carve + prune")
    # carving alone, out of place
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **CARVE)
    pc, poses, removed = step_loop(gs, slam, frames_of(gs, s, s["depths"]), inplace=False)
    assert [int(r[0]) for r in removed] == moved[3] and pc._carve_steps == L_SEQ
    same_as_oracle(pc, poses, moved[1], moved[2], "out of place, carve")


def test_depth_residual_shows_the_ghost_and_its_removal(gs, moved, stepped):
    from gradslam_amd.metrics import depth_residual
    s, m, oposes, _, plain = moved
    pc = stepped[0]
    Kc = s["intrinsics"][0]
    last = frames_of(gs, s, s["depths"])[:, L_SEQ - 1]
    posed = gs.RGBDImages(last.rgb_image, last.depth_image, last.intrinsics, dev(oposes[None, -1:]))
    got = depth_residual(pc, posed)
    ref_carved = rr.residual_stats(rr.render(m.points, m.normals, m.colors, m.ccounts, oposes[-1], Kc, cr.SEQ_H, cr.SEQ_W).depth,
                                   s["depths"][-1])
    ref_plain = rr.residual_stats(rr.render(plain.points, plain.normals, plain.colors, plain.ccounts, oposes[-1], Kc,
                                            cr.SEQ_H, cr.SEQ_W).depth, s["depths"][-1])
    print("rmse of the last model view: uncarved", ref_plain["rmse"], "carved", ref_carved["rmse"])
    assert float(got["coverage"][0, 0]) == ref_carved["coverage"] == 1.0
    assert float(got["rmse"][0, 0]) == pytest.approx(ref_carved["rmse"], rel=1e-9)   # float64 sums of <= H * W terms
    # the table's effect: the ghost costs 0.1 m of RMSE, the carved map is back at the millimetres of a clean run
    assert ref_plain["rmse"] > 0.1 and ref_carved["rmse"] < 0.01
    assert cr.ghost_rows(m.points, s["clean"][-1], oposes[-1], Kc) == 0
    assert cr.ghost_rows(plain.points, s["clean"][-1], oposes[-1], Kc) > 600
