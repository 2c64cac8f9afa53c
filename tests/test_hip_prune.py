"""GPU tests of the map prune (gs_prune.hip -> gs_prune_map_dc_f32 -> ops.prune_map_batch -> Pointclouds.prune_ ->
PointFusion(prune_*=...)) against its NumPy restatement (tests/prune_ref.py) and, end to end, against the oracle frame
loop that applies the restatement between frames.

The prune moves bits (rows are copied as 32-bit words) and the step is bit-identical to the oracle, so every comparison
is for EQUAL BITS: no tolerance anywhere.  Tile = 1024 rows, wave = 64, the tile scan is one block of 1024 threads: the row
counts sit on and around those sizes, and 1024 * 1024 + 5 rows make the tile scan loop."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from oracle import slam as oslam
from tests import prune_ref as pr
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
SENT = 0x7FC0DEAD   # a NaN payload no input holds: destination rows the prune must not write keep it
TILE = 1024
BIG = 1024 * 1024 + 5


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


_ROWS = {}


def rows(n, F=1, seed=0):
    """points / normals / colors of random BITS (NaN payloads, denormals, -0 included: they must arrive unchanged) and
    features in [0, 1); computed once per size and never changed"""
    key = (n, F, seed)
    if key not in _ROWS:
        rng = np.random.default_rng(1000 + seed)
        raw = lambda c: rng.integers(0, 1 << 32, size=(n, c), dtype=np.uint64).astype(np.uint32).view(np.float32)  # noqa: E731
        arrs = (raw(3), raw(3), raw(3), rng.random((n, F), dtype=np.float32))
        for a in arrs[:3]:
            assert not (bits(a) == SENT).any()
        _ROWS[key] = arrs
    return _ROWS[key]


def pattern(name, n, seed=0):
    s = np.zeros(n, dtype=bool)
    if name == "all":
        s[:] = True
    elif name == "alternate":
        s[::2] = True
    elif name == "row0":
        s[:1] = True
    elif name == "last":
        s[n - 1:] = True
    elif name == "tile_removed":     # one whole tile removed between two kept ones (what fits into n)
        s[:] = True
        s[TILE:2 * TILE] = False
    elif name == "random":
        s = np.random.default_rng(seed).random(n) < 0.5
    else:
        assert name == "none"
    return s


PATTERNS = ("none", "all", "alternate", "row0", "last", "tile_removed", "random")


def sentinel(shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def run_one(ops, arrs, n, *, cap_extra=7, n_bound=None, min_confidence=None, keep=None, marks=None, young_mark=-1):
    """ops.prune_map_batch for one map into sentinel-filled destinations of capacity above n_bound; checks every
    destination row against the restatement (rows below the new count) or the sentinel (all the others), the counts and
    the marks.  arrs: four arrays of >= n_bound rows (None: attribute absent).  Returns the restatement's result."""
    n_bound = n if n_bound is None else n_bound
    src = [None if a is None else dev(a[:n_bound]) for a in arrs]
    cap = n_bound + cap_extra
    out = [None if a is None else sentinel((cap, a.shape[1])) for a in arrs]
    n_dev = None if n_bound == n else torch.tensor([n], dtype=torch.int64, device="cuda")
    mk = None if marks is None else torch.tensor(marks, dtype=torch.int64, device="cuda")
    r = ops.prune_map_batch([tuple(src) + (n_bound, n_dev)], min_confidence=min_confidence,
                            keep=None if keep is None else [dev(keep[:n_bound])], marks=None if mk is None else [mk],
                            young_mark=young_mark, out=[out])
    want = pr.prune(*arrs, n, min_confidence, keep, marks if marks is not None else (), young_mark)
    k = want[4]
    assert r.counts.dtype == torch.int64 and r.counts.is_cuda and tuple(r.counts.shape) == (1,)
    assert host(r.counts).tolist() == [k] and host(r.removed).tolist() == [want[5]]
    for name, o, w in zip("PNCF", r.maps[0], want[:4]):
        assert (o is None) == (w is None), name
        if o is None:
            continue
        assert o.shape[0] == cap
        assert np.array_equal(bits(host(o[:k])), bits(w)), "%s: rows below the new count" % name
        assert bool((o[k:].view(torch.int32) == SENT).all()), "%s: a row at or beyond the new count was written" % name
    if marks is not None:
        assert host(mk).tolist() == want[6]
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, BIG])
def test_kernel_equals_restatement(ops, n):
    P, N, C, F = rows(n)
    for name in PATTERNS:
        s = pattern(name, n, seed=n)
        # through the confidence rule (survivors hold a confidence at or above the threshold) ...
        cc = np.where(s[:, None], np.maximum(F, np.float32(0.5)), np.minimum(F, np.float32(0.49))).astype(np.float32)
        want = run_one(ops, (P, N, C, cc), n, min_confidence=0.5)
        assert want[4] == int(s.sum()), name
        # ... and through keep (bool)
        want = run_one(ops, (P, N, C, F), n, keep=s)
        assert want[4] == int(s.sum()), name
    # both rules at once: a row needs both
    if n:
        keep = pattern("random", n, seed=n + 1).astype(np.uint8) * 3
        want = run_one(ops, (P, N, C, F), n, min_confidence=0.5, keep=keep)
        assert want[4] == int(((F[:, 0] >= 0.5) & (keep != 0)).sum())


def test_rows_beyond_the_device_count_never_survive(ops):
    n, extra = 2049, 3000
    P, N, C, F = rows(n + extra, seed=1)
    F = F.copy()
    F[n:] = 1.0                                  # would pass the rule
    keep = np.ones(n + extra, np.uint8)          # and keep
    want = run_one(ops, (P, N, C, F), n, n_bound=n + extra, min_confidence=0.5, keep=keep, marks=[0, n, n + 10, n + extra],
                   young_mark=-1)
    assert 0 < want[4] < n and want[6][1:] == [want[4]] * 3
    # a device count above the bound is clamped to the bound
    src = [dev(a) for a in (P, N, C, F)]
    r = ops.prune_map_batch([tuple(src) + (n, torch.tensor([n + 50], dtype=torch.int64, device="cuda"))], min_confidence=0.5)
    assert host(r.counts).tolist() == [want[4]]


def test_threshold_equality_nan_and_young_rows(ops):
    n = 200
    P, N, C, _ = rows(n, seed=2)
    th = np.float32(0.3)
    F = np.full((n, 1), th, np.float32)
    F[1::4] = np.nextafter(th, np.float32(0))    # one ulp below: removed
    F[2::4] = np.nan                             # removed
    F[3::4] = np.inf
    want = run_one(ops, (P, N, C, F), n, min_confidence=float(th))
    assert want[4] == n // 2
    # young rows are exempt (the NaN among them too); old ones are not
    want = run_one(ops, (P, N, C, F), n, min_confidence=float(th), marks=[100, 150], young_mark=0)
    assert want[4] == 50 + 100 and want[6] == [50, 100]
    # a threshold that rounds to th in float32
    run_one(ops, (P, N, C, F), n, min_confidence=float(th) + 1e-10)
    # negative zero passes a threshold of zero
    Z = np.zeros((n, 1), np.float32)
    Z[::2] = -0.0
    assert run_one(ops, (P, N, C, Z), n, min_confidence=0.0)[4] == n


def test_absent_attributes_and_wide_features(ops):
    n = 1025
    P, N, C, F = rows(n, seed=3)
    s = pattern("random", n, seed=5)
    run_one(ops, (P, None, None, F), n, min_confidence=0.5)
    run_one(ops, (P, None, C, None), n, keep=s)
    run_one(ops, (P, N, None, F), n, keep=s, min_confidence=0.25)
    P3, N3, C3, F3 = rows(n, F=3, seed=4)
    want = run_one(ops, (P3, N3, C3, F3), n, keep=s)
    assert want[3].shape == (int(s.sum()), 3)
    with pytest.raises(ValueError, match="one feature channel"):
        ops.prune_map(dev(P3), dev(N3), dev(C3), dev(F3), min_confidence=0.5)
    # default destinations: new tensors of the sources' shapes
    r = ops.prune_map(dev(P), dev(N), dev(C), dev(F), keep=dev(s))
    k = int(s.sum())
    assert [tuple(t.shape) for t in r.maps] == [(n, 3), (n, 3), (n, 3), (n, 1)]
    assert np.array_equal(bits(host(r.maps[0][:k])), bits(P[s])) and host(r.counts).tolist() == [k]


def test_the_library_rejects_in_place(ops):
    from gradslam_amd import _C
    P, N, C, F = [dev(a) for a in rows(100, seed=6)]
    with pytest.raises(_C.HipExtensionError, match="alias"):
        ops.prune_map(P, N, C, F, min_confidence=0.5, out=(torch.empty_like(P), N, torch.empty_like(C), torch.empty_like(F)))


@pytest.mark.parametrize("counts", [(1025, 0, 70001), (5, 1024, 2049, 0, 3000, 1, 4097, 64, 70001)])
def test_batch_equals_single_calls(ops, counts):
    """B = 3 in one launch group and B = 9 in two: every sequence as in a call of its own, and as the restatement"""
    B = len(counts)
    srcs, keeps, marks, singles = [], [], [], []
    for b, n in enumerate(counts):
        P, N, C, F = rows(n, seed=10 + b)
        srcs.append([dev(a) for a in (P, N, C, F)])
        keeps.append(None if b % 2 else dev(pattern("random", n, seed=b) | (np.arange(n) % 5 == 0)))
        marks.append([0, n // 3, n // 2, n])
        want = pr.prune(P, N, C, F, n, 0.3, None if keeps[b] is None else host(keeps[b]), marks[b], 2)
        mk1 = torch.tensor(marks[b], dtype=torch.int64, device="cuda")
        one = ops.prune_map(*srcs[b], min_confidence=0.3, keep=keeps[b], marks=mk1, young_mark=2)
        assert host(one.counts).tolist() == [want[4]] and host(mk1).tolist() == want[6]
        for o, w in zip(one.maps, want[:4]):
            assert np.array_equal(bits(host(o[:want[4]])), bits(w))
        singles.append((one, mk1, want))
    mk = [torch.tensor(m, dtype=torch.int64, device="cuda") for m in marks]
    got = ops.prune_map_batch([tuple(srcs[b]) + (counts[b], None) for b in range(B)], min_confidence=0.3, keep=keeps,
                              marks=mk, young_mark=2)
    assert tuple(got.counts.shape) == (B,) and tuple(got.removed.shape) == (B,)
    assert host(got.counts).tolist() == [w[4] for _, _, w in singles]
    assert host(got.removed).tolist() == [w[5] for _, _, w in singles]
    for b, (one, mk1, want) in enumerate(singles):
        k = want[4]
        for o, o1 in zip(got.maps[b], one.maps):
            assert torch.equal(o[:k].view(torch.int32), o1[:k].view(torch.int32)), b
        assert torch.equal(mk[b], mk1), b


def test_marks_and_two_prunes_in_a_row(ops):
    n = 2500
    P, N, C, F = rows(n, seed=20)
    marks = [0, 1024, 1500, 1500, 2048, n, n + 100]     # 0, tile borders, mid-tile, duplicates, n, beyond n
    for ym in range(-1, len(marks)):
        want = run_one(ops, (P, N, C, F), n, min_confidence=0.5, marks=marks, young_mark=ym)
        assert want[6] == sorted(want[6]) and want[6][0] == 0 and want[6][-1] == want[4]
    assert run_one(ops, (P, N, C, F), n, min_confidence=0.5, marks=marks, young_mark=0)[4] == n   # every row young
    # 64 marks, the most a call takes
    many = sorted(np.random.default_rng(3).integers(0, n + 50, 64).tolist())
    run_one(ops, (P, N, C, F), n, min_confidence=0.5, marks=many, young_mark=40)
    # the second prune starts from the first one's rows and marks
    a = run_one(ops, (P, N, C, F), n, min_confidence=0.4, marks=marks, young_mark=4)
    b = run_one(ops, a[:4], a[4], min_confidence=0.7, marks=a[6], young_mark=2)
    assert 0 < b[4] < a[4] < n


# ------------------------------------------------------------------------------------------ Pointclouds
def device_map(gs, counts, seed=30, extra=500):
    """a Pointclouds whose counts live on the device (one group), on buffers with `extra` rows of room whose contents
    would pass every rule"""
    B = len(counts)
    pc = gs.Pointclouds(device="cuda")
    pc._init_empty_batch(B, 1)
    arrs = []
    for b, n in enumerate(counts):
        P, N, C, F = rows(n + extra, seed=seed + b)
        F = F.copy()
        F[n:] = 9.0
        arrs.append((P, N, C, F))
        for k, a in zip(("points", "normals", "colors", "features"), (P, N, C, F)):
            pc._buf[k][b] = dev(a)
    # bounds = counts + extra, with no read-back in flight that could tighten them behind the test's back
    cnt = torch.tensor(counts, dtype=torch.int64, device="cuda")
    pc._n_host[:] = list(counts)
    pc._set_counts_dev(cnt, 0)
    pc._set_counts_dev(cnt, extra)
    torch.cuda.synchronize()
    pc._dcount[0].group.poll()
    assert pc._dcount[0].group.bounds == [n + extra for n in counts] and not pc._dcount[0].group._pending
    return pc, arrs


def test_pointclouds_prune_leaves_the_counts_on_the_device(gs):
    counts = (3000, 1, 1500)
    pc, arrs = device_map(gs, counts)
    assert len(pc._dcount) == 3 and [pc._count_of(b)[0] for b in range(3)] == [n + 500 for n in counts]
    pc.mark_epoch()
    bounds = list(pc._dcount[0].group.bounds)
    caps = [t.shape[0] for t in pc._buf["points"]]
    gen = pc._generation
    pc.prune_(0.5, keep=[torch.arange(counts[0], device="cuda") % 3 != 0] +
              [torch.ones(counts[b], dtype=torch.bool) for b in (1, 2)])
    assert len(pc._dcount) == 3, "the prune resolved a device-side count"
    assert pc._dcount[0].group.bounds == bounds, "the bounds change only when a read-back lands"
    assert [t.shape[0] for t in pc._buf["points"]] == caps and pc._generation > gen
    assert pc.last_pruned.is_cuda
    want = []
    for b, n in enumerate(counts):
        keep = (np.arange(n) % 3 != 0) if b == 0 else np.ones(n, bool)
        want.append(pr.prune(*arrs[b], n, 0.5, keep, [n], -1))
    assert pc._tighten_counts() == [w[4] for w in want]
    assert len(pc._dcount) == 3
    assert host(pc.last_pruned).tolist() == [w[5] for w in want]
    assert host(pc._marks[:, 0]).tolist() == [w[6][0] for w in want]
    for b, w in enumerate(want):
        for k, a in zip(("points", "normals", "colors", "features"), w[:4]):
            assert np.array_equal(bits(host(pc._buf[k][b][:w[4]])), bits(a)), (b, k)
    # the lists (which resolve the counts) agree
    assert [t.shape[0] for t in pc.points_list] == [w[4] for w in want]


def test_pointclouds_prune_with_host_counts_and_min_age(gs):
    ns = (1500, 0, 700)
    lists = [[dev(rows(n, seed=40 + b)[i]) for b, n in enumerate(ns)] for i in range(4)]
    pc = gs.Pointclouds(*lists)
    cuts = ([500, 0, 100], [1000, 0, 650], list(ns))
    for c in cuts:
        pc._n_host[:] = c
        pc.mark_epoch()
    assert pc._n_host == list(ns)
    pc.prune_(0.6, min_age=4)                      # more epochs than recorded: nothing goes
    assert pc._n == list(ns) and host(pc.last_pruned).tolist() == [0, 0, 0]
    pc.prune_(0.6, min_age=2)
    for b, n in enumerate(ns):
        w = pr.prune(*rows(n, seed=40 + b), n, 0.6, None, [c[b] for c in cuts], 1)
        assert pc._n[b] == w[4] and host(pc._marks[b, :3]).tolist() == w[6]
        assert np.array_equal(bits(host(pc.points_list[b])), bits(w[0]))
        assert np.array_equal(bits(host(pc.features_list[b])), bits(w[3]))
    out = pc.prune(0.9)
    assert out is not pc and sum(out._n) < sum(pc._n) and out._n_marks == 3


# ------------------------------------------------------------------------------------------ end to end
L, H, W = 8, 96, 128
PRUNE = dict(prune_min_confidence=0.004, prune_min_age=2, prune_every=2)


@pytest.fixture(scope="module")
def scene():
    """the 8-frame 96x128 sequence and the oracle loop that prunes with the restatement after steps 3, 5 and 7 (0-based;
    the prune that falls on step 1 finds fewer than two marks and removes nothing), each prune before that step's mark"""
    s = make_sequence(L, H, W, seed=0)
    marks, log = [], []

    def per_frame(i, m, pose):
        if (i + 1) % PRUNE["prune_every"] == 0 and len(marks) >= PRUNE["prune_min_age"]:
            out = pr.prune(m.points, m.normals, m.colors, m.ccounts, len(m), PRUNE["prune_min_confidence"], None, marks,
                           len(marks) - PRUNE["prune_min_age"])
            log.append((i, len(m), out[4]))
            m.points, m.normals, m.colors, m.ccounts = out[:4]
            marks[:] = out[6]
        marks.append(len(m))

    m, poses = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gradicp", per_frame=per_frame)
    plain, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gradicp")
    print("oracle prunes (step, rows before, rows after):", log, "final", len(m), "unpruned", len(plain))
    assert [i for i, _, _ in log] == [3, 5, 7]
    assert all(0 < after < before for _, before, after in log), log
    assert len(m) < len(plain)
    return s, m, poses, log, marks


def frames_of(gs, s):
    poses = T(s["poses"][None]).cuda()
    poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)


def same_as_oracle(pts, nrm, col, cc, poses, m, oposes, what):
    assert pts.shape == m.points.shape, (what, pts.shape, m.points.shape)
    for name, a, b in (("points", pts, m.points), ("normals", nrm, m.normals), ("colors", col, m.colors),
                       ("ccounts", cc, m.ccounts), ("poses", poses, oposes)):
        assert np.array_equal(a, b), "%s %s: %d of %d differ" % (what, name, (a != b).sum(), a.size)


@pytest.fixture(scope="module")
def stepped(gs, scene):
    """the sequence stepped in place with the pruning PointFusion (fast path from the third frame on)"""
    s = scene[0]
    frames = frames_of(gs, s)
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **PRUNE)
    pc, prev, rec, removed = gs.Pointclouds(device="cuda"), None, [], []
    for i in range(L):
        live = frames[:, i]
        pc, p = slam.step(pc, live, prev, inplace=True)
        prev = live
        rec.append(host(p[0, 0]))
        if i % 2 == 1:
            removed.append(int(pc.last_pruned[0]))
    assert getattr(slam, "_step_plan", None) is not None, "the in-place loop must have taken the fast path"
    assert len(pc._dcount) == 1, "the counts stay on the device through the prunes"
    return pc, np.stack(rec), removed, frames


def test_pruning_slam_equals_the_pruning_oracle(scene, stepped):
    s, m, oposes, log, omarks = scene
    pc, poses, removed, _ = stepped
    assert removed == [0] + [before - after for _, before, after in log]
    assert pc._prune_steps == L and pc._n_marks == L
    assert host(pc._marks[0, :L]).tolist() == omarks
    same_as_oracle(*[host(x[0]) for x in (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)], poses, m,
                   oposes, "fast path")


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from gradslam_amd.datasets.synthetic import make_sequence
s = make_sequence(8, 96, 128, seed=0)
T = torch.from_numpy
poses = T(s["poses"][None]).cuda(); poses[:, 1:] = poses[:, :1]
frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
slam = gs.slam.PointFusion(odom="gradicp", device="cuda", prune_min_confidence=0.004, prune_min_age=2, prune_every=2)
pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
for i in range(8):
    live = frames[:, i]
    pc, p = slam.step(pc, live, prev, inplace=True)
    prev = live
    rec.append(p[0, 0].cpu().numpy())
assert getattr(slam, "_step_plan", None) is None, "GRADSLAM_HIP_FASTPATH=0 must keep the fast path out"
np.savez(sys.argv[1], poses=np.stack(rec), pts=pc.points_list[0].cpu().numpy(), nrm=pc.normals_list[0].cpu().numpy(),
         col=pc.colors_list[0].cpu().numpy(), cc=pc.features_list[0].cpu().numpy())
"""


def test_generic_path_prunes_the_same(scene, tmp_path):
    s, m, oposes, _, _ = scene
    out = str(tmp_path / "generic.npz")
    subprocess.run([sys.executable, "-c", _CHILD % REPO, out], check=True, timeout=600,
                   env=dict(os.environ, GRADSLAM_HIP_FASTPATH="0"))
    z = np.load(out)
    same_as_oracle(z["pts"], z["nrm"], z["col"], z["cc"], z["poses"], m, oposes, "generic path")


def test_forward_prunes_the_same(gs, scene):
    s, m, oposes, _, _ = scene
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", **PRUNE)
    pc, poses = slam(frames_of(gs, s))
    same_as_oracle(*[host(x[0]) for x in (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)],
                   host(poses[0]), m, oposes, "forward")


def test_render_and_residual_on_the_pruned_map(gs, scene, stepped):
    from gradslam_amd.metrics import depth_residual
    s, m, oposes, _, _ = scene
    pc, _, _, frames = stepped
    K = s["intrinsics"][0]
    view = dev(oposes[None, 5:6])
    rendered, extras = pc.render(frames.intrinsics, view, H, W, return_extras=True)
    want = rr.render(m.points, m.normals, m.colors, m.ccounts, oposes[5], K, H, W)
    assert (want.index >= 0).mean() > 0.1 and want.index.max() < len(m)
    for got, ref in ((rendered.depth_image[0, 0], want.depth), (rendered.rgb_image[0, 0], want.color),
                     (extras["normal"][0, 0], want.normal), (extras["confidence"][0, 0], want.confidence),
                     (extras["index"][0, 0], want.index)):
        assert np.array_equal(host(got), ref)
    posed = gs.RGBDImages(frames.rgb_image, frames.depth_image, frames.intrinsics, dev(oposes[None]))
    got = depth_residual(pc, posed)
    for f in range(L):
        r = rr.render(m.points, m.normals, m.colors, m.ccounts, oposes[f], K, H, W)
        ref = rr.residual_stats(r.depth, s["depths"][f])
        assert float(got["coverage"][0, f]) == ref["coverage"] and float(got["pixels"][0, f]) == ref["pixels"]
        for k in ("mean_abs", "median_abs", "rmse"):   # float64 sums of <= H * W terms (tests/test_hip_render.py)
            assert float(got[k][0, f]) == pytest.approx(ref[k], rel=1e-9), (f, k)


def test_backward_of_a_render_taken_before_a_prune_raises(gs):
    pc, _ = device_map(gs, (3000,), seed=50, extra=0)
    pose = torch.eye(4, device="cuda").view(1, 1, 4, 4).clone().requires_grad_(True)
    K = torch.tensor([[60.0, 0, 32, 0], [0, 60.0, 24, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device="cuda").view(1, 1, 4, 4)
    pc._buf["points"][0] = dev(rows(3000, seed=50)[3].repeat(3, 1) + np.float32(0.5))   # in front of the camera
    stale = pc.render(K, pose, 48, 64, differentiable=True).depth_image.sum()
    pc.prune_(0.5)
    with pytest.raises(RuntimeError, match="changed in place"):
        stale.backward()
