"""GPU tests of the feature layers: gs_fuse_features_batch and gs_compact_features_batch bit for bit against the NumPy
restatement (tests/feature_fuse_ref.py) on the tables of the real map update, held to their scratch and their buffers by
guard bands (tests/scratch_guard.py), and the PointFusion drivers with a layer against a hand-written loop of existing
calls, against the run without the fast path and against the run without a layer."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from tests import feature_fuse_cases as cases
from tests import feature_fuse_ref as ref
from tests import scratch_guard as sg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_TH, DOT_TH, SIGMA = 0.05, math.cos(20 * math.pi / 180), 0.6
SIZES = ((6, 7), (17, 19), (33, 65))             # 33 x 65 = 2145 pixels: two 1024-element compaction tiles and a rest
CHANNELS = (1, 3, 4, 5, 8, 20, 64, 260)          # both sides of the 16-byte rule for float32 and for float16
MASKS = ("none", "zero", "checker", "nofeat")
DTYPES = {"f32": (torch.float32, np.float32), "f16": (torch.float16, np.float16)}
FILL = 0x5A


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------ the tables of a real update
@functools.lru_cache(maxsize=None)
def tables(H, W, B):
    """B sequences: frame 0 builds the maps, frame 1 is updated into them with want_best_pix=True.  Host copies of what
    the feature pass runs on and of what it is checked against (computed once, read-only)."""
    from gradslam_amd import ops
    P = H * W
    seqs = [make_sequence(2, H, W, seed=20 + b, hole_frac=0.1 + 0.02 * b) for b in range(B)]
    K = dev(np.stack([s["intrinsics"][0] for s in seqs]))
    bufs = [[torch.zeros((3 * P + 64, k), device="cuda") for k in (3, 3, 3, 1)] for _ in range(B)]
    counts = [0] * B
    for f in range(2):
        depth = dev(np.stack([s["depths"][f, ..., 0] for s in seqs]))
        rgb = dev(np.stack([s["colors"][f] for s in seqs]))
        pose = dev(np.stack([s["poses"][f] for s in seqs]))
        v, n, a = ops.frame_maps_batch(depth.view(B, 1, H, W), K, SIGMA)
        maps = [ops.MapRows(*bufs[b], counts[b], None) for b in range(B)]
        n_old = list(counts)
        cnt, gv, _, best = ops.update_map_fusion_batch_(maps, v[:, 0], n[:, 0], depth, rgb, a[:, 0], pose, K, DIST_TH, DOT_TH,
                                                        want_best_pix=True)
        counts = [int(c) for c in host(cnt)]
    t = dict(depth=host(depth), alpha=host(a[:, 0]), best=host(best), n_old=n_old, n_new=counts, gv=host(gv),
             points=[host(bufs[b][0]) for b in range(B)])
    for x in t.values():
        for y in (x if isinstance(x, list) else [x]):
            if isinstance(y, np.ndarray):
                y.setflags(write=False)
    return t


def layer_state(rng, rows, Cn, npdt):
    """the layer before the pass: some rows never fused (weight 0, zeros), the rest random"""
    emb = (rng.standard_normal((rows, Cn)) * 3).astype(npdt)
    weight = (rng.random(rows) * 5).astype(np.float32)
    empty = rng.random(rows) < 0.1
    emb[empty] = 0
    weight[empty] = 0
    return emb, weight


def mask_of(kind, P, W):
    if kind == "zero":
        return np.zeros(P, np.uint8)
    if kind == "checker":
        return ((np.arange(P) // W + np.arange(P) % W) % 2).astype(np.uint8)
    return None


def guarded_layer(log, b, cap, Cn, tdt, emb0, w0):
    """emb (cap, C) and weight (cap,) between guard bands; the first rows hold emb0 / w0, the rest the fill"""
    es = 4 if tdt == torch.float32 else 2
    emb = sg.guarded_buffer(log, "emb%d" % b, cap * Cn * es, "cuda").view(tdt).view(cap, Cn)
    weight = sg.guarded_buffer(log, "weight%d" % b, cap * 4, "cuda").view(torch.float32)
    emb[:emb0.shape[0]] = dev(emb0)
    weight[:w0.shape[0]] = dev(w0)
    return emb, weight


def run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, kind, *, best="table", n_dev_below=0, slack=0, depth=None):
    """one call of ops.fuse_features_batch on guarded buffers under the exact workspace, compared with the restatement;
    returns the device results"""
    tdt, npdt = DTYPES[dt]
    P = H * W
    rng = np.random.default_rng(1000 * Cn + H)
    depth_h = t["depth"] if depth is None else depth
    best_h = best if not isinstance(best, str) else (t["best"] if best == "table" else None)
    feat_h = None if kind == "nofeat" else (rng.standard_normal((B, H, W, Cn)) * 2).astype(npdt)
    valid_h = mask_of(kind, P, W)
    log = sg.GuardLog(FILL)
    layers, want, n_old = [], [], []
    for b in range(B):
        n_true = t["n_old"][b] - n_dev_below
        bound = t["n_old"][b] + slack
        cap = bound + P                                   # the least the entry accepts
        emb0, w0 = layer_state(rng, bound, Cn, npdt)
        layers.append(guarded_layer(log, b, cap, Cn, tdt, emb0, w0))
        before_e, before_w = host(layers[b][0]), host(layers[b][1])
        n_old.append((bound, dev(np.array([n_true], np.int64)) if (n_dev_below or slack) else None))
        want.append(ref.fuse(before_e, before_w, n_true, None if best_h is None else best_h[b], depth_h[b], t["alpha"][b],
                             None if feat_h is None else feat_h[b], valid_h))
    with sg.exact_scratch(monkeypatch, FILL) as ws_log:
        r = ops.fuse_features_batch(layers, n_old, None if best_h is None else dev(best_h), dev(depth_h), dev(t["alpha"]),
                                    None if feat_h is None else dev(feat_h),
                                    None if valid_h is None else dev(np.stack([valid_h] * B)))
        torch.cuda.synchronize()
        assert sg.intact(ws_log) == (True, []) and [n for n, _ in sg.requests(ws_log)] == ["scratch"]
        from gradslam_amd import _C
        assert sg.requests(ws_log)[0][1] == sum(_C.lib().gs_scratch_bytes(nb, P) for nb, _ in n_old)
    assert sg.intact(log) == (True, []), sg.intact(log)
    rows, cnt = host(r.row_of_pix), host(r.counts)
    for b in range(B):
        emb_w, wgt_w, rows_w, n_w = want[b]
        what = (b, Cn, dt, kind)
        assert cnt[b] == n_w, what
        assert np.array_equal(rows[b], rows_w), what
        # the whole buffers: rows at or beyond the count are as they were (the restatement leaves them alone)
        assert same_bits(host(layers[b][0]), emb_w), what
        assert same_bits(host(layers[b][1]), wgt_w), what
    return r, layers, want


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("H,W", SIZES)
def test_the_pass_alone_equals_the_restatement(ops, monkeypatch, H, W, B):
    t = tables(H, W, B)
    P = H * W
    for b in range(B):
        matched = ((t["best"][b] >= 0) & (t["best"][b] < t["n_old"][b])).sum()
        assert matched > 0 and t["n_new"][b] > t["n_old"][b], "the frame must both match and append"
    first = True
    for Cn in CHANNELS:
        for dt in DTYPES:
            for kind in MASKS:
                r, layers, want = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, kind)
                if first:
                    first = False
                    rows = host(r.row_of_pix)
                    for b in range(B):
                        # the new count is the map's own, and the restated append order is the real one: the map row of
                        # every appended pixel holds that pixel's global vertex
                        assert int(r.counts[b]) == t["n_new"][b]
                        app = np.nonzero(rows[b] >= t["n_old"][b])[0]
                        assert app.size == t["n_new"][b] - t["n_old"][b] > 0
                        assert same_bits(t["points"][b][rows[b][app]], t["gv"][b].reshape(P, 3)[app])
                    # two runs give the same bits
                    r2, layers2, _ = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, kind)
                    assert torch.equal(r2.row_of_pix, r.row_of_pix)
                    assert all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(layers, layers2))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_frames_without_a_match_without_an_append_and_without_a_table(ops, monkeypatch, dt):
    H, W, B = 17, 19, 3
    t = tables(H, W, B)
    for Cn in (5, 8):
        none = np.full_like(t["best"], -1)
        r, _, _ = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, "none", best=none)              # no match
        assert bool((r.row_of_pix[0] < t["n_old"][0]).logical_and(r.row_of_pix[0] >= 0).sum() == 0)
        no_app = np.where(t["best"].reshape(B, H, W) < 0, np.float32(0), t["depth"]).astype(np.float32)
        r, _, _ = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, "checker", depth=no_app)        # no append
        assert [int(c) for c in r.counts] == t["n_old"]
        r, _, _ = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, "none", best="none")            # best_pix = NULL
        assert [int(c) for c in r.counts] == [t["n_old"][b] + int((t["depth"][b] > 0).sum()) for b in range(B)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_stale_entries_and_a_device_count_below_its_bound(ops, monkeypatch, dt):
    H, W, B = 33, 65, 2
    t = tables(H, W, B)
    best = t["best"].copy()
    best[:, 3] = 0x7fffffff                       # the tie marker: none
    best[:, 5] = np.array(t["n_old"]) + 2         # beyond the old count: none
    below = 40                                    # the device count is 40 below the map's: its last 40 rows turn stale
    assert all(((best[b] >= t["n_old"][b] - below) & (best[b] < t["n_old"][b])).any() for b in range(B))
    for Cn in (3, 64):
        r, _, want = run_pass(ops, monkeypatch, t, B, H, W, Cn, dt, "none", best=best, n_dev_below=below, slack=100)
        rows = host(r.row_of_pix)
        for b in range(B):
            assert rows[b][3] == -1 and rows[b][5] == -1
            stale = (best[b] >= t["n_old"][b] - below) & (best[b] >= 0)
            assert (rows[b][stale] == -1).all()


def test_every_buffer_of_the_c_entry_is_held_to_its_size(ops):
    """the C entry on buffers of exactly the documented sizes, each between guard bands: emb, weight, row_of_pix, n_out and
    gs_scratch_bytes(n_old_bound, H * W) of scratch per sequence; two fills give the same bits (nothing is read before
    it is written)"""
    from gradslam_amd import _C
    H, W, B, Cn = 33, 65, 9, 24              # 48 bytes per row: the 16-byte path
    t = tables(H, W, B)
    P = H * W
    L = _C.lib()
    rng = np.random.default_rng(4)
    feat = dev((rng.standard_normal((B, H, W, Cn)) * 2).astype(np.float16))
    depth, alpha, best = dev(t["depth"]), dev(t["alpha"]), dev(t["best"])
    state = [layer_state(rng, t["n_old"][b], Cn, np.float16) for b in range(B)]
    results = []
    for fill in (0x00, 0xFF):
        log = sg.GuardLog(fill)
        seqs = (_C.FeatureFuseSeq * B)()
        keep = []
        for b in range(B):
            cap = t["n_old"][b] + P
            emb, weight = guarded_layer(log, b, cap, Cn, torch.float16, *state[b])
            rows = sg.guarded_buffer(log, "rows%d" % b, 4 * P, "cuda")
            n_out = sg.guarded_buffer(log, "n_out%d" % b, 8, "cuda")
            scratch = sg.guarded_buffer(log, "scratch%d" % b, L.gs_scratch_bytes(t["n_old"][b], P), "cuda")
            keep.append((emb, weight, rows, n_out, scratch))
            u = seqs[b]
            u.emb, u.weight, u.capacity = emb.data_ptr(), weight.data_ptr(), cap
            u.n_old_bound, u.n_old_dev = t["n_old"][b], 0
            u.best_pix, u.depth, u.alpha = (x[b].data_ptr() for x in (best, depth, alpha))
            u.feat, u.valid = feat[b].data_ptr(), 0
            u.row_of_pix, u.n_out, u.scratch = rows.data_ptr(), n_out.data_ptr(), scratch.data_ptr()
        _C.check(L.gs_fuse_features_batch(seqs, B, H, W, Cn, _C.FEATURE_F16, _C.stream(torch.device("cuda", 0))), "fuse")
        torch.cuda.synchronize()
        assert sg.intact(log) == (True, []), sg.intact(log)
        results.append([(host(k[0][:t["n_new"][b]]), host(k[1][:t["n_new"][b]]), host(k[2]), host(k[3]))
                        for b, k in enumerate(keep)])
    for b in range(B):
        assert all(same_bits(x, y) for x, y in zip(results[0][b], results[1][b])), b
        assert int(results[0][b][3].view(np.int64)[0]) == t["n_new"][b]


# ------------------------------------------------------------------------------------------ the compaction alone
def keep_patterns(rng, n):
    out = dict(all=np.ones(n, np.uint8), none=np.zeros(n, np.uint8), alternate=(np.arange(n) % 2).astype(np.uint8),
               random=(rng.random(n) < 0.6).astype(np.uint8) * 3)               # (any non-zero byte keeps)
    edge = np.zeros(n, np.uint8)
    edge[[1023, 1024]] = 1                                                     # one row either side of a tile boundary
    out["boundary"] = edge
    return out


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("Cn", [1, 5, 8, 260])
def test_the_compaction_alone_equals_the_restatement_and_the_map_prune(ops, monkeypatch, dt, Cn):
    tdt, npdt = DTYPES[dt]
    rng = np.random.default_rng(Cn)
    n = 2500
    pats = keep_patterns(rng, n)
    for name, keep in pats.items():
        for below in (0, 300):                       # n_dev below n_bound: the rows behind it never survive
            emb, weight = layer_state(rng, n, Cn, npdt)
            weight = np.arange(n, dtype=np.float32)   # (the row's own index: what the map prune is compared on)
            n_true = n - below
            log = sg.GuardLog(FILL)
            src = guarded_layer(log, 0, n, Cn, tdt, emb, weight)
            dst = guarded_layer(log, 1, n, Cn, tdt, emb[:0], weight[:0])
            n_dev = dev(np.array([n_true], np.int64)) if below else None
            with sg.exact_scratch(monkeypatch, FILL) as ws_log:
                r = ops.compact_features_batch([src], [(n, n_dev)], [dev(keep)], out=[dst])
                torch.cuda.synchronize()
                assert sg.intact(ws_log) == (True, [])
            assert sg.intact(log) == (True, [])
            e_w, w_w, c_w = ref.compact(emb, weight, keep, n_true)
            what = (name, below)
            assert int(r.counts[0]) == c_w, what
            assert same_bits(host(dst[0][:c_w]), e_w) and same_bits(host(dst[1][:c_w]), w_w), what
            # destination rows at or beyond the count are not written
            assert (bits(host(dst[0][c_w:])) == bits(np.frombuffer(bytes([FILL] * 4), npdt)[:1])[0]).all(), what
            assert (bits(host(dst[1][c_w:])) == 0x5A5A5A5A).all(), what
            # the map's prune with the same mask keeps the same rows
            pts = dev(np.repeat(np.arange(n, dtype=np.float32)[:, None], 3, 1))
            pm = ops.prune_map_batch([(pts, None, None, None, n, n_dev)], keep=[dev(keep)])
            assert int(pm.counts[0]) == c_w and np.array_equal(host(pm.maps[0][0][:c_w, 0]), w_w), what


def test_compaction_of_nine_layers_of_different_sizes(ops, monkeypatch):
    rng = np.random.default_rng(9)
    sizes = [1, 1023, 1024, 1025, 2048, 3000, 7, 2500, 4097]
    for dt, (tdt, npdt) in DTYPES.items():
        Cn = 8 if dt == "f32" else 5
        log = sg.GuardLog(FILL)
        srcs, dsts, keeps, state = [], [], [], []
        for b, n in enumerate(sizes):
            emb, weight = layer_state(rng, n, Cn, npdt)
            keep = (rng.random(n) < 0.5).astype(np.uint8)
            state.append((emb, weight, keep))
            srcs.append(guarded_layer(log, 2 * b, n, Cn, tdt, emb, weight))
            dsts.append(guarded_layer(log, 2 * b + 1, n, Cn, tdt, emb[:0], weight[:0]))
            keeps.append(dev(keep))
        with sg.exact_scratch(monkeypatch, FILL) as ws_log:
            r = ops.compact_features_batch(srcs, [(n, None) for n in sizes], keeps, out=dsts)
            torch.cuda.synchronize()
            assert sg.intact(ws_log) == (True, [])
        assert sg.intact(log) == (True, [])
        for b, n in enumerate(sizes):
            e_w, w_w, c_w = ref.compact(*state[b], n)
            assert int(r.counts[b]) == c_w
            assert same_bits(host(dsts[b][0][:c_w]), e_w) and same_bits(host(dsts[b][1][:c_w]), w_w), (dt, b)


# ------------------------------------------------------------------------------------------ the drivers
MAP_KEYS = ("n", "pts", "nrm", "col", "cc", "poses")
LAYER_KEYS = ("emb", "wgt")


def equal_runs(a, b, keys, what):
    for k in keys:
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@functools.lru_cache(maxsize=None)
def step_runs():
    return cases.step_runs()


@pytest.mark.parametrize("odom", cases.ODOMS)
def test_step_forward_and_hand_written_loop_agree(odom):
    step = step_runs()[odom + "_f16"]
    assert bool(step["fast"]) == (odom == "gradicp")            # (the one-call step serves icp / gradicp)
    assert step["emb"].shape == (int(step["n"].sum()), cases.C) and step["wgt"].shape == (int(step["n"].sum()),)
    equal_runs(step, cases.run_forward(odom, torch.float16), MAP_KEYS + LAYER_KEYS, "forward")
    equal_runs(step, cases.run_hand(odom, torch.float16), MAP_KEYS + LAYER_KEYS, "hand-written loop")
    equal_runs(step, cases.run_steps(odom, torch.float16, layer=False), MAP_KEYS, "without a layer")
    # features on every second frame only, under a mask, float32
    second = step_runs()[odom + "_f32_second_masked"]
    equal_runs(second, cases.run_hand(odom, torch.float32, every=2, masked=True), MAP_KEYS + LAYER_KEYS, "every second")
    equal_runs(second, step, MAP_KEYS, "the map does not depend on the layer")
    assert (second["wgt"] == 0).any() and (second["wgt"] > 0).any()


def test_fast_path_equals_generic_path_with_a_layer(tmp_path):
    """the `step` runs again in a fresh child process with GRADSLAM_HIP_FASTPATH=0: same bits in the map and the layer"""
    out = str(tmp_path / "generic.npz")
    subprocess.run([sys.executable, "-m", "tests.feature_fuse_cases", out], check=True, timeout=600, cwd=REPO,
                   env=dict(os.environ, GRADSLAM_HIP_FASTPATH="0"))
    generic = np.load(out)
    here = cases.flat(step_runs())
    assert set(generic.files) == set(here)
    for k in sorted(here):
        if k.endswith("/fast"):
            assert not bool(generic[k])
        else:
            assert same_bits(np.asarray(here[k]), generic[k]), k
    assert bool(here["gradicp_f16/fast"])


@pytest.mark.parametrize("odom", cases.ODOMS)
def test_weight_is_the_confidence_count_through_prune_carve_and_thinning(odom):
    seen = []

    def per_step(pc, layer, s):
        n = [int(t.shape[0]) for t in pc.points_list]
        assert [int(t.shape[0]) for t in layer.features_list] == n == [int(t.shape[0]) for t in layer.weights_list]
        for b in range(cases.B):
            assert torch.equal(layer.weights_list[b].view(torch.int32), pc.features_list[b][:, 0].view(torch.int32)), (s, b)
        seen.append((n, None if pc.last_pruned is None else host(pc.last_pruned).tolist()))

    out = cases.run_steps(odom, torch.float16, per_step=per_step, **cases.SCHEDULES)
    assert len(seen) == cases.L and any(p is not None and sum(p) > 0 for _, p in seen), seen     # rows were removed
    # the schedule run that never reads the lists between steps (device-side counts throughout) ends the same
    equal_runs(out, step_runs()[odom + "_f16_schedules"], MAP_KEYS + LAYER_KEYS, "per-step reads")


def test_depth_filter_and_outlier_mask_reach_the_pass():
    """the pass sees the frame the map update saw: the filtered copy, and with fuse_outliers=False the masked one"""
    for odom, kw in (("gradicp", dict(depth_filter=dict(radius=1))),
                     ("projicp", dict(odom_outlier_mask=dict(), fuse_outliers=False))):
        def per_step(pc, layer, s):
            for b in range(cases.B):
                assert torch.equal(layer.weights_list[b].view(torch.int32), pc.features_list[b][:, 0].view(torch.int32))
        cases.run_steps(odom, torch.float32, per_step=per_step, **kw)


def test_a_feature_image_that_requires_grad_warns_and_the_layer_is_detached():
    import gradslam_amd as gs
    frames, feats, _ = cases.inputs(torch.float32)
    slam = cases.slam_of("gradicp")
    pc = gs.Pointclouds(device="cuda").attach_features(gs.MapFeatures(cases.C))
    f = feats[:, 0].clone().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        slam.step(pc, frames[:, 0], None, inplace=True, features=f)
    assert not pc.map_features.features_list[0].requires_grad
