"""The feature-layer rule without a GPU: the NumPy restatement (tests/feature_fuse_ref.py) against the oracle's frame
loop and against exact rational arithmetic, the restated compaction, the exports, every refusal of the two C entry points
(before any HIP call) and the refusals of the Python layer."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _C, ops
from gradslam_amd.datasets.synthetic import make_sequence
from gradslam_amd.slam import ICPSLAM, PointFusion
from oracle import oracle as o
from tests import feature_fuse_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_TH, DOT_TH, SIGMA = 0.05, math.cos(20 * math.pi / 180), 0.6
L, H, W = 6, 60, 80
f32, f16 = np.float32, np.float16


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ the oracle's frame loop
@functools.lru_cache(maxsize=None)
def frame_loop(scene, renorm):
    """per frame: the tables the feature pass runs on and the oracle's map after the update (computed once, read-only)"""
    seq = make_sequence(L, H, W, seed=0, scene=scene)
    K = seq["intrinsics"][0]
    e3, e1 = np.zeros((0, 3), f32), np.zeros((0, 1), f32)
    P, N, Cc, F = e3, e3, e3, e1
    frames = []
    for s in range(L):
        depth, rgb, pose = seq["depths"][s, ..., 0], seq["colors"][s], seq["poses"][s]
        v, n, a, _ = o.frame_maps(depth, K, SIGMA)
        gv, gn = o.global_maps(v, n, depth, pose)
        if P.shape[0]:
            pix = o.project_map(P, pose, K, H, W)
            best, _ = o.associate(pix, P, N, F, gv, gn, DIST_TH, DOT_TH)
            best = o.rows_to_best_pix(o.best_table(best, H, W), H, W)
        else:
            best = np.full(H * W, -1, np.int32)
        n_old = P.shape[0]
        P, N, Cc, F = o.fuse_append(P, N, Cc, F, best, gv, gn, rgb, a, depth, renorm_all=renorm)
        fr = dict(best=best, depth=depth, alpha=a, rgb=rgb, n_old=n_old, colors=Cc, ccounts=F[:, 0].copy(), n_new=P.shape[0])
        for k, t in fr.items():
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
        frames.append(fr)
    return tuple(frames)


def run_layer(frames, dtype, feats=None, valids=None, C=3):
    """the restatement applied after every frame; feats[s] None: feat = NULL; yields (frame, emb, weight, rows)"""
    cap = frames[-1]["n_new"] + 1
    emb = np.full((cap, C), 7, dtype)      # (rows at or beyond the count keep this filling)
    weight = np.full(cap, 7, f32)
    for s, fr in enumerate(frames):
        feat = fr["rgb"].astype(dtype) if feats is None else feats[s]
        valid = None if valids is None else valids[s]
        emb, weight, rows, n_new = ref.fuse(emb, weight, fr["n_old"], fr["best"], fr["depth"], fr["alpha"], feat, valid)
        assert n_new == fr["n_new"]
        assert (bits(emb[n_new:]) == bits(np.full(1, 7, dtype))[0]).all() and (weight[n_new:] == 7).all()
        yield fr, emb, weight, rows


@pytest.mark.parametrize("scene", ["wave", "facets"])
def test_rgb_as_feature_equals_the_maps_colours_and_weights_the_counts(scene):
    frames = frame_loop(scene, False)
    assert frames[1]["n_new"] > frames[0]["n_new"] and (frames[1]["best"] >= 0).sum() > 1000   # matches and appends
    for fr, emb, weight, _ in run_layer(frames, f32):
        n = fr["n_new"]
        assert same_bits(emb[:n], fr["colors"]), "colours"
        assert same_bits(weight[:n], fr["ccounts"]), "counts"


@pytest.mark.parametrize("scene", ["wave", "facets"])
def test_weight_equals_the_confidence_count_with_renormalisation(scene):
    for fr, _, weight, _ in run_layer(frame_loop(scene, True), f32):
        assert same_bits(weight[:fr["n_new"]], fr["ccounts"])


# ------------------------------------------------------------------------------------------ exact arithmetic
def rne(x, p, emin):
    """the binary floating-point number of precision p (minimum exponent emin) nearest to the Fraction x >= 0, ties to
    even, as a Fraction"""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    q, r = divmod(x, quantum)
    if r * 2 > quantum or (r * 2 == quantum and q % 2 == 1):
        q += 1
    return q * quantum


def r32(x):
    return rne(x, 24, -126)


def merged_exact(w, e, a, f, half):
    """((w * e) + (a * f)) * (1 / (w + a)), one rounding per operation, in exact rational arithmetic"""
    w, e, a, f = (Fraction(float(t)) for t in (w, e, a, f))
    w2 = r32(w + a)
    inv = r32(1 / (w2 if w2 != 0 else Fraction(1)))
    out = r32(r32(r32(w * e) + r32(a * f)) * inv)
    return rne(out, 11, -14) if half else out


def test_rne_helper_against_numpy():
    rng = np.random.default_rng(5)
    for x in rng.random(200) * 300:
        assert float(r32(Fraction(float(x)))) == float(f32(x))
        assert float(rne(Fraction(float(x)), 11, -14)) == float(f16(x))
    assert float(rne(Fraction(3, 2 ** 26), 11, -14)) == float(f16(3 / 2 ** 26))      # (a float16 subnormal)


def test_rows_appended_under_a_zero_mask_are_zero_and_a_later_match_gives_them_the_pinned_value():
    frames = frame_loop("wave", True)[:2]
    P = H * W
    runs = list(run_layer(frames, f32, valids=[np.zeros(P, np.uint8), None]))
    fr0, emb0, w0, _ = runs[0]
    n0 = fr0["n_new"]
    assert (bits(emb0[:n0]) == 0).all() and (bits(w0[:n0]) == 0).all()             # +0 and +0.0, not -0
    fr1, emb1, w1, rows = runs[1]
    pm = np.nonzero((rows >= 0) & (rows < n0))[0]
    assert pm.size > 1000
    a = fr1["alpha"].reshape(-1)[pm]
    f = fr1["rgb"].reshape(P, 3)[pm]
    want = (a[:, None] * f) * (f32(1.0) / a)[:, None]                                # 0 * 0 + a f, times 1 / (0 + a)
    assert want.dtype == f32 and same_bits(emb1[rows[pm]], want) and same_bits(w1[rows[pm]], a)
    exact = bits(want) == bits(f)
    assert exact.any() and not exact.all()          # both kinds occur: the feature itself, and the pinned neighbour
    assert same_bits(emb1[rows[pm]][exact], f[exact])
    for i in range(0, pm.size, 97):                 # ... and in exact arithmetic, operation by operation
        for c in range(3):
            assert Fraction(float(emb1[rows[pm[i]], c])) == merged_exact(0.0, 0.0, a[i], f[i, c], False)


@pytest.mark.parametrize("half", [False, True])
def test_merged_rows_are_pinned_by_exact_arithmetic(half):
    frames = frame_loop("facets", True)[:3]
    dtype = f16 if half else f32
    runs = list(run_layer(frames, dtype))
    (_, emb1, w1, _), (fr2, emb2, w2, rows) = runs[1], runs[2]
    P = H * W
    pm = np.nonzero((rows >= 0) & (rows < fr2["n_old"]))[0]
    a = fr2["alpha"].reshape(-1)
    f = fr2["rgb"].astype(dtype).reshape(P, 3)
    assert pm.size > 1000
    for p in pm[::53]:
        r = rows[p]
        for c in range(3):
            assert Fraction(float(emb2[r, c])) == merged_exact(w1[r], emb1[r, c], a[p], f[p, c], half)
        assert Fraction(float(w2[r])) == r32(Fraction(float(w1[r])) + Fraction(float(a[p])))


def test_float16_layer_is_the_float32_one_rounded_once_on_appended_rows():
    frames = frame_loop("wave", True)
    last32 = list(run_layer(frames, f32))[-1]
    last16 = list(run_layer(frames, f16))[-1]
    fr = frames[-1]
    assert fr["n_new"] > fr["n_old"]
    rows = np.arange(fr["n_old"], fr["n_new"])          # appended by the last frame: never merged
    assert same_bits(last16[1][rows], last32[1][rows].astype(f16))
    assert same_bits(last16[2], last32[2])              # the weights are float32 either way


def test_feat_null_creates_the_rows_and_a_checkerboard_leaves_matched_rows_alone():
    frames = frame_loop("wave", True)[:3]
    P = H * W
    board = ((np.arange(P) // W + np.arange(P) % W) % 2).astype(np.uint8)
    feats = [frames[0]["rgb"], None, frames[2]["rgb"]]
    runs = list(run_layer(frames, f32, feats=feats, valids=[None, None, board]))
    (_, e0, w0, _), (fr1, e1, w1, _), (fr2, e2, w2, rows2) = runs
    n0, n1 = fr1["n_old"], fr1["n_new"]
    assert same_bits(e1[:n0], e0[:n0]) and same_bits(w1[:n0], w0[:n0])         # feat = NULL: matched rows untouched
    assert (bits(e1[n0:n1]) == 0).all() and (bits(w1[n0:n1]) == 0).all()       # ... and the appended rows exist, empty
    off = np.nonzero((rows2 >= 0) & (rows2 < n1) & (board == 0))[0]
    assert off.size > 100 and same_bits(e2[rows2[off]], e1[rows2[off]]) and same_bits(w2[rows2[off]], w1[rows2[off]])


def test_rows_of_pixels_edges():
    depth = np.array([1, 0, 2, 1, -1, np.nan, 3, 1], f32)
    best = np.array([-1, -1, 0x7fffffff, 5, -1, -1, 2, -1], np.int32)          # a tie marker, a stale entry (n_old = 5)
    rows, n_new = ref.rows_of_pixels(best, depth, 5)
    assert rows.tolist() == [5, -1, -1, -1, -1, -1, 2, 6] and n_new == 7
    rows, n_new = ref.rows_of_pixels(None, depth, 5)                           # best_pix = NULL: every pixel with depth
    assert rows.tolist() == [5, -1, 6, 7, -1, -1, 8, 9] and n_new == 10


def test_restated_compaction_is_boolean_mask_indexing():
    rng = np.random.default_rng(3)
    for dtype, Cn in ((f32, 5), (f16, 8)):
        emb = rng.standard_normal((3000, Cn)).astype(dtype)
        weight = rng.random(3000).astype(f32)
        keep = (rng.random(3000) < 0.4).astype(np.uint8)
        e, w, cnt = ref.compact(emb, weight, keep, 2500)
        assert cnt == int(keep[:2500].sum())
        assert same_bits(e, emb[:2500][keep[:2500] != 0]) and same_bits(w, weight[:2500][keep[:2500] != 0])
    conf = np.array([0.5, np.nan, 2.0, 1.0, 0.1], f32)
    assert ref.keep_of_rule(conf, 5, None, 1.0, None).tolist() == [False, False, True, True, False]
    assert ref.keep_of_rule(conf, 5, [1, 1, 0, 1, 1], 1.0, 4).tolist() == [False, False, False, True, True]


# ------------------------------------------------------------------------------------------ the C entry points
NEW = ("gs_fuse_features_batch", "gs_compact_features_batch")


def test_exports_and_header():
    assert set(NEW) <= set(_C.EXPORTS)
    with open(os.path.join(REPO, "include", "gradslam_hip.h")) as fh:
        header = fh.read()
    lib = _C.lib()
    for n in NEW:
        assert hasattr(lib, n) and re.search(r"GS_API int %s\(" % n, header), n
    assert not any(n.endswith("_scratch_bytes") or n.startswith("gs_projective_icp_") for n in NEW)


def fuse_seq(**kw):
    """a descriptor that passes every check for H x W = 6 x 7 (fake aligned pointers: nothing is dereferenced before a HIP
    call, and every case below is rejected before one)"""
    names = ("emb", "weight", "n_old_dev", "best_pix", "depth", "alpha", "feat", "valid", "row_of_pix", "n_out", "scratch")
    a = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}
    a.update(capacity=142, n_old_bound=100)
    a.update(kw)
    q = _C.FeatureFuseSeq()
    for k, v in a.items():
        setattr(q, k, v)
    return q


def compact_seq(**kw):
    names = ("emb", "weight", "n_dev", "keep", "emb_out", "weight_out", "n_out", "scratch")
    a = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}
    a.update(n_bound=100, capacity_out=100)
    a.update(kw)
    q = _C.FeatureCompactSeq()
    for k, v in a.items():
        setattr(q, k, v)
    return q


def call_fuse(q, B=1, H=6, W=7, C=4, dtype=0):
    return _C.lib().gs_fuse_features_batch(None if q is None else C_ptr(q), B, H, W, C, dtype, None)


def call_compact(q, B=1, C=4, dtype=0):
    return _C.lib().gs_compact_features_batch(None if q is None else C_ptr(q), B, C, dtype, None)


def C_ptr(q):
    return C.pointer(q)


FUSE_INVALID = {
    "null_descriptors": (None, {}, "NULL"),
    "no_sequences": ({}, dict(B=0), "B <= 0"),
    "null_emb": (dict(emb=0), {}, "NULL"),
    "null_weight": (dict(weight=0), {}, "NULL"),
    "null_depth": (dict(depth=0), {}, "NULL"),
    "null_alpha": (dict(alpha=0), {}, "NULL"),
    "null_row_of_pix": (dict(row_of_pix=0), {}, "NULL"),
    "null_n_out": (dict(n_out=0), {}, "NULL"),
    "null_scratch": (dict(scratch=0), {}, "NULL"),
    "no_channels": ({}, dict(C=0), "C must be"),
    "too_many_channels": ({}, dict(C=4097), "C must be"),
    "unknown_dtype": ({}, dict(dtype=2), "dtype"),
    "negative_dtype": ({}, dict(dtype=-1), "dtype"),
    "capacity_one_short": (dict(capacity=141), {}, "capacity"),
    "negative_bound": (dict(n_old_bound=-1), {}, "n_old_bound"),
    "misaligned_emb": (dict(emb=0x100008), {}, "aligned"),
    "misaligned_feat_on_the_vector_path": (dict(feat=0x700004), {}, "aligned"),
    "feat_is_emb": (dict(feat=0x100000), {}, "alias"),
    "no_rows": ({}, dict(H=0), "sizes"),
    "negative_columns": ({}, dict(W=-7), "sizes"),
    "two_to_the_31_pixels": (dict(capacity=1 << 40), dict(H=1 << 16, W=1 << 15), "2^31"),
    "rows_beyond_int32": (dict(capacity=1 << 40, n_old_bound=(1 << 31) - 42), {}, "2^31"),
}
COMPACT_INVALID = {
    "null_descriptors": (None, {}, "NULL"),
    "no_sequences": ({}, dict(B=0), "B <= 0"),
    "null_emb": (dict(emb=0), {}, "NULL"),
    "null_weight": (dict(weight=0), {}, "NULL"),
    "null_keep": (dict(keep=0), {}, "NULL"),
    "null_emb_out": (dict(emb_out=0), {}, "NULL"),
    "null_weight_out": (dict(weight_out=0), {}, "NULL"),
    "null_n_out": (dict(n_out=0), {}, "NULL"),
    "null_scratch": (dict(scratch=0), {}, "NULL"),
    "no_channels": ({}, dict(C=0), "C must be"),
    "too_many_channels": ({}, dict(C=4097), "C must be"),
    "unknown_dtype": ({}, dict(dtype=7), "dtype"),
    "capacity_one_short": (dict(capacity_out=99), {}, "capacity"),
    "negative_bound": (dict(n_bound=-1), {}, "n_bound"),
    "misaligned_emb": (dict(emb=0x100004), {}, "aligned"),
    "misaligned_emb_out": (dict(emb_out=0x500002), {}, "aligned"),
    "emb_out_is_emb": (dict(emb_out=0x100000), {}, "alias"),
    "weight_out_is_weight": (dict(weight_out=0x200000), {}, "alias"),
}


@pytest.mark.parametrize("case", sorted(FUSE_INVALID))
def test_fuse_entry_rejects_before_any_hip_call(case):
    change, args, word = FUSE_INVALID[case]
    assert call_fuse(None if change is None else fuse_seq(**change), **args) == 1          # GS_ERR_INVALID
    msg = _C.lib().gs_last_error().decode()
    assert msg.startswith("gs_fuse_features_batch") and word in msg, msg


@pytest.mark.parametrize("case", sorted(COMPACT_INVALID))
def test_compact_entry_rejects_before_any_hip_call(case):
    change, args, word = COMPACT_INVALID[case]
    assert call_compact(None if change is None else compact_seq(**change), **args) == 1
    msg = _C.lib().gs_last_error().decode()
    assert msg.startswith("gs_compact_features_batch") and word in msg, msg


def test_a_misaligned_feat_is_fine_on_the_scalar_path_up_to_the_next_check():
    # C = 5 float32: 20 bytes per row, no 16-byte units; the descriptor then fails a later check only
    assert call_fuse(fuse_seq(feat=0x700004, capacity=141), C=5) == 1
    assert "capacity" in _C.lib().gs_last_error().decode()


def test_feature_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_features.hip", "gs_ff_", "gs_fc_"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln and not ln.startswith("#")]
    assert len(rows) == 12, r.stdout          # count, scan, rows, 4 fuse instances; count, scan, 3 scatter instances
    for row in rows:
        assert row[2] == "0" and row[4] == "0" and row[5] == "0", row        # scratch, SGPR spills, VGPR spills


# ------------------------------------------------------------------------------------------ the Python layer
def cpu_map(n=(5, 7)):
    g = torch.Generator().manual_seed(1)
    mk = lambda c: [torch.rand((k, c), generator=g) for k in n]      # noqa: E731
    return gs.Pointclouds(mk(3), mk(3), mk(3), mk(1))


def cpu_frame(B=2, h=6, w=8):
    seq = make_sequence(1, h, w, seed=0)
    st = lambda k: torch.from_numpy(np.stack([seq[k]] * B))            # noqa: E731
    return gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), st("poses").unsqueeze(1)[:, :, 0:1].reshape(B, 1, 4, 4))


def test_layer_constructor_and_attachment():
    for bad in (0, 4097, -1):
        with pytest.raises(ValueError):
            gs.MapFeatures(bad)
    with pytest.raises(TypeError):
        gs.MapFeatures(3.0)
    with pytest.raises(ValueError):
        gs.MapFeatures(3, torch.bfloat16)
    pc, layer = cpu_map(), gs.MapFeatures(4, torch.float16)
    assert pc.map_features is None and pc.attach_features(layer) is pc and pc.map_features is layer
    # the rows the map already holds: zeros with weight 0
    assert [tuple(t.shape) for t in layer.features_list] == [(5, 4), (7, 4)] and layer.features_list[0].dtype == torch.float16
    assert all(bool((t == 0).all()) for t in layer.features_list + layer.weights_list)
    with pytest.raises(ValueError, match="already has a feature layer"):
        pc.attach_features(gs.MapFeatures(4))
    with pytest.raises(ValueError, match="another pointclouds"):
        cpu_map().attach_features(layer)
    with pytest.raises(TypeError):
        cpu_map().attach_features("layer")
    # copies come without it
    assert pc.clone().map_features is None and pc[0].map_features is None and pc.prune(0.5).map_features is None
    assert pc.detach_features() is layer and pc.map_features is None and pc.detach_features() is None
    with pytest.raises(ValueError, match="not attached"):
        layer.features_list


def test_calls_that_would_change_rows_behind_the_layer_raise():
    pc = cpu_map().attach_features(gs.MapFeatures(3))
    with pytest.raises(ValueError, match="feature layer"):
        pc.append_points(cpu_map())
    for name in ("points", "normals", "colors", "features"):
        with pytest.raises(ValueError, match="feature layer"):
            setattr(pc, name + "_list", getattr(pc, name + "_list"))
        with pytest.raises(ValueError, match="feature layer"):
            setattr(pc, name + "_padded", getattr(pc, name + "_padded"))
    live = cpu_frame()
    with pytest.raises(ValueError, match="feature layer"):
        ICPSLAM(odom="gt").step(pc, live, None, inplace=True)
    with pytest.raises(ValueError, match="inplace=True"):
        PointFusion(odom="gt").step(pc, live, None, inplace=False)
    with pytest.raises(ValueError, match="inplace=True"):
        PointFusion(odom="gt").step(pc, live, None)
    pc.detach_features()
    pc.append_points(cpu_map())                                   # (without the layer everything is as before)
    with pytest.raises(ValueError, match="no feature layer"):
        PointFusion(odom="gt").step(pc, live, None, inplace=True, features=torch.zeros(2, 6, 8, 3))


def test_step_refuses_wrong_feature_images_before_it_touches_the_map():
    pc = cpu_map().attach_features(gs.MapFeatures(3))
    live, slam = cpu_frame(), PointFusion(odom="gt")
    before = [t.clone() for t in pc.points_list]
    ok = torch.zeros(2, 6, 8, 3)
    for bad, err in ((torch.zeros(2, 6, 8, 4), ValueError), (torch.zeros(2, 8, 6, 3), ValueError),
                     (torch.zeros(1, 6, 8, 3), ValueError), (torch.zeros(2, 2, 6, 8, 3), ValueError),
                     (ok.half(), ValueError), (ok.double(), ValueError), (ok.numpy(), TypeError)):
        with pytest.raises(err, match="features"):
            slam.step(pc, live, None, inplace=True, features=bad)
    for bad, err in ((torch.ones(2, 6, 9, dtype=torch.bool), ValueError), (torch.ones(2, 6, 8), TypeError)):
        with pytest.raises(err, match="features_valid"):
            slam.step(pc, live, None, inplace=True, features=ok, features_valid=bad)
    with pytest.raises(ValueError, match="without features"):
        slam.step(pc, live, None, inplace=True, features_valid=torch.ones(2, 6, 8, dtype=torch.bool))
    assert all(torch.equal(a, b) for a, b in zip(before, pc.points_list))
    with pytest.raises(ValueError, match="features"):
        slam.forward(live, features=torch.zeros(2, 1, 6, 9, 3))
    with pytest.raises(ValueError, match="without features"):
        slam.forward(live, feature_dtype=torch.float16)


def test_ops_refuse_cpu_tensors_and_wrong_layers():
    emb, weight = torch.zeros(100, 4), torch.zeros(100)
    depth = torch.ones(1, 6, 7)
    with pytest.raises(_C.HipExtensionError, match="GPU only"):
        ops.fuse_features_batch([(emb, weight)], [(10, None)], None, depth, depth, torch.zeros(1, 6, 7, 4))
    with pytest.raises(_C.HipExtensionError, match="GPU only"):
        ops.compact_features_batch([(emb, weight)], [(100, None)], [torch.ones(100, dtype=torch.uint8)])
    for layers in ([], [(emb.double(), weight)], [(emb, weight.half())], [(emb, weight[:50])], [(emb.view(-1), weight)],
                   [(emb, weight), (emb.half(), weight)], [(emb, weight), (torch.zeros(100, 5), weight)]):
        with pytest.raises(ValueError):
            ops.fuse_features_batch(layers, [(10, None)] * len(layers), None, depth.expand(max(len(layers), 1), 6, 7),
                                    depth.expand(max(len(layers), 1), 6, 7))
    with pytest.raises(ValueError, match="feat must"):
        ops.fuse_features_batch([(emb, weight)], [(10, None)], None, depth, depth, torch.zeros(1, 6, 7, 5))
    with pytest.raises(ValueError, match="dtype"):
        ops.fuse_features_batch([(emb, weight)], [(10, None)], None, depth, depth, torch.zeros(1, 6, 7, 4).half())
    with pytest.raises(ValueError, match="best_pix"):
        ops.fuse_features_batch([(emb, weight)], [(10, None)], torch.zeros(1, 42, dtype=torch.int64), depth, depth)
    with pytest.raises(ValueError, match="keep"):
        ops.compact_features_batch([(emb, weight)], [(100, None)], [torch.ones(99, dtype=torch.uint8)])


def test_cpu_prune_indexes_the_layer_with_the_maps_selection():
    pc = cpu_map((40, 50))
    layer = gs.MapFeatures(6)
    pc.attach_features(layer)
    g = torch.Generator().manual_seed(2)
    for b in range(2):
        layer._emb[b][:] = torch.rand(layer._emb[b].shape, generator=g)
        layer._weight[b][:] = torch.rand(layer._weight[b].shape, generator=g)
    emb = [t.clone() for t in layer.features_list]
    wgt = [t.clone() for t in layer.weights_list]
    conf = [t[:, 0].clone() for t in pc.features_list]
    keep = [torch.rand(40, generator=g) < 0.7, torch.rand(50, generator=g) < 0.7]
    pc.prune_(0.3, keep=keep)
    for b in range(2):
        s = torch.from_numpy(ref.keep_of_rule(conf[b].numpy(), conf[b].shape[0], keep[b].numpy(), 0.3, None))
        assert 0 < int(s.sum()) < s.shape[0]
        assert torch.equal(layer.features_list[b], emb[b][s]) and torch.equal(layer.weights_list[b], wgt[b][s])
        assert layer.features_list[b].shape[0] == pc.points_list[b].shape[0]


def test_similarity_and_gather_are_plain_torch():
    pc = cpu_map((4, 3))
    layer = gs.MapFeatures(2)
    pc.attach_features(layer)
    layer._emb[0][:4] = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, 3.0], [5.0, 0.0]])
    layer._weight[0][:4] = torch.tensor([1.0, 1.0, 2.0, 0.0])
    s = layer.similarity(torch.tensor([2.0, 0.0]))
    assert torch.allclose(s[0], torch.tensor([1.0, 0.0, 2 ** -0.5, 0.0])) and tuple(s[1].shape) == (3,)   # weight 0 scores 0
    s2 = layer.similarity(torch.tensor([[2.0, 0.0], [0.0, 1.0]]))
    assert tuple(s2[0].shape) == (4, 2) and torch.allclose(s2[0][:, 1], torch.tensor([0.0, 1.0, 2 ** -0.5, 0.0]))
    with pytest.raises(ValueError):
        layer.similarity(torch.zeros(3))
    idx = torch.tensor([[[[0, -1], [2, 1]]], [[[-1, -1], [-1, -1]]]])
    img = layer.gather(idx)
    assert tuple(img.shape) == (2, 1, 2, 2, 2)
    assert img[0, 0].tolist() == [[[1.0, 0.0], [0.0, 0.0]], [[3.0, 3.0], [0.0, 2.0]]] and bool((img[1] == 0).all())
    with pytest.raises(ValueError):
        layer.gather(torch.zeros(2, 1, 2, 2))
