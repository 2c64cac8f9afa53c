"""CPU tests of the projective ICP's outlier mask: the NumPy restatement (tests/outlier_mask_ref.py) -- the properties of
the rule, what the mask and the refinement without it are worth on the 60 x 80 scenes (the README's table, to the
restatement's own digits) -- and, without a GPU, the exports, the argument checks of the C entry points (made before any
HIP call) and of the Python layers, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import outlier_mask_ref as om
from tests import picp_ref as pr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr
from tests import picp_weighted_ref as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("gs_picp_outlier_classes_scratch_bytes", "gs_picp_outlier_classes_batch_f32", "gs_region_mask_u8")
S, E = om.STRONG | om.ELIGIBLE, om.ELIGIBLE       # the class bytes of a strong and of a merely eligible pixel


# ------------------------------------------------------------------------------------------ the rule
def random_classes(shape, seed, p_strong=0.35, p_eligible=0.3):
    """uint8 class images: strong (3), eligible only (2) or nothing (0); never strong without eligible"""
    u = np.random.default_rng(seed).uniform(size=shape)
    return np.where(u < p_strong, S, np.where(u < p_strong + p_eligible, E, 0)).astype(np.uint8)


def random_depth(shape, seed):
    """float32 depths around 1 m in steps that straddle the default grow_depth, with holes"""
    rng = np.random.default_rng(seed)
    d = (1.0 + 0.015 * rng.integers(0, 4, shape)).astype(F)
    d[rng.uniform(size=shape) < 0.05] = 0
    return d


def test_grow_zero_gives_the_seeds_and_the_support_counts_the_window():
    cls = random_classes((23, 31), 1)
    d = random_depth((23, 31), 2)
    strong = (cls & om.STRONG) != 0
    for k in (1, 4, 6, 9):
        m = om.region_mask(cls, d, k, 0)
        assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        assert np.array_equal(m != 0, om.seeds(cls, k))
        for y, x in ((0, 0), (0, 30), (22, 0), (11, 17), (22, 30)):       # the window by hand; outside counts as not strong
            n = strong[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum()
            assert bool(m[y, x]) == bool(strong[y, x] and n >= k), (k, y, x)
    assert np.array_equal(om.region_mask(cls, d, 1, 0) != 0, strong)                 # min_support 1: every strong pixel
    assert not om.region_mask(cls, d, 9, 0)[[0, -1]].any()                           # a border pixel never has nine
    full = np.full((5, 6), S, np.uint8)
    assert om.region_mask(full, np.ones((5, 6), F), 9, 0)[1:-1, 1:-1].all()


def test_the_mask_is_monotone_in_grow_and_never_leaves_the_eligible_pixels():
    cls = random_classes((37, 53), 3)
    d = random_depth((37, 53), 4)
    prev = om.region_mask(cls, d, 6, 0)
    assert prev.any()
    for g in range(1, 17):
        m = om.region_mask(cls, d, 6, g)
        assert (m >= prev).all()
        assert not m[(cls & om.ELIGIBLE) == 0].any()              # class-0 pixels are never masked
        prev = m
    assert prev.sum() > om.region_mask(cls, d, 6, 0).sum()


@pytest.mark.parametrize("grow", [0, 1, 3, 16])
def test_a_corridor_is_reached_up_to_step_grow_and_no_further(grow):
    cls, d = corridor(grow, 3, 40)
    m = om.region_mask(cls, d, 1, grow)
    want = np.zeros_like(cls)
    want[3, 2:2 + grow + 1] = 1
    assert np.array_equal(m, want)
    # ... and downwards, the same corridor transposed
    assert np.array_equal(om.region_mask(cls.T.copy(), d.T.copy(), 1, grow), want.T)


def corridor(grow, row, width, x0=2):
    """one seed at (row, x0) and grow + 2 merely eligible pixels to its right, in an image of 7 x width"""
    cls = np.zeros((7, width), np.uint8)
    cls[row, x0] = S
    cls[row, x0 + 1:x0 + grow + 3] = E
    return cls, np.ones((7, width), F)


def test_the_depth_gap_is_closed_at_equality_and_open_above():
    cls = np.zeros((3, 4), np.uint8)
    cls[1, 0], cls[1, 1:] = S, E
    d = np.ones((3, 4), F)
    d[1, 1] = F(1.25)                                               # |1.25 - 1| == 0.25 exactly
    d[1, 2] = np.nextafter(F(1.25), F(2))                           # ... and one float32 above
    d[1, 3] = d[1, 2]
    assert F(d[1, 2] - F(1)) > F(0.25)
    m = om.region_mask(cls, d, 1, 3, 0.25)
    assert m[1].tolist() == [1, 1, 1, 1]                            # 1.25 -> next: a gap of one ulp, far below 0.25
    d[1, 1] = d[1, 2]
    assert om.region_mask(cls, d, 1, 3, 0.25)[1].tolist() == [1, 0, 0, 0]
    d[1, 1] = np.nan                                                # a NaN depth is never reached
    assert om.region_mask(cls, d, 1, 3, 0.25)[1].tolist() == [1, 0, 0, 0]
    assert om.region_mask(cls, d, 1, 3, np.inf)[1].tolist() == [1, 0, 0, 0]


def test_classes_follow_the_codes_and_strict_comparisons():
    code = np.array([0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 0], np.int32)
    b = np.array([0.003, -0.003, 0.0015, 0.001, 9, 9, 9, 0, 0, 9, np.nan], F)
    c = om.classes(code, b, F(0.003), F(0.0015))
    assert c.tolist() == [E, E, 0, 0, 0, 0, 0, S, S, 0, 0]          # equality is not above; a NaN residual is no outlier
    c = om.classes(code, b, F(0.002), F(0.001))
    assert c.tolist() == [S, S, E, 0, 0, 0, 0, S, S, 0, 0]
    c = om.classes(code, b, F(0), F(0))                             # a threshold of 0: nothing by its residual
    assert c.tolist() == [0, 0, 0, 0, 0, 0, 0, S, S, 0, 0]


def test_thresholds_are_the_scale_rule_and_an_empty_view_masks_nothing():
    fx = rr.moved_block(pr.convergence_fixture())
    for floor in (0.0, 0.03):
        out = om.outliers(*pr.args_of(fx), fx["T0"], hi=3.0, lo=1.5, floor=floor)
        used = out.code.reshape(-1) == 0
        b = out.b.reshape(-1)
        assert out.thresholds.dtype == F and used.sum() > 3000
        assert out.thresholds[0] == sr.scale(b, used, 3.0, floor) and out.thresholds[1] == sr.scale(b, used, 1.5, floor)
        assert np.array_equal(out.classes, om.classes(out.code, out.b, *out.thresholds))
        assert not out.mask[~np.isin(out.code, (0, 4, 5))].any()
    assert out.thresholds[1] == F(0.03) < out.thresholds[0]       # the floor took the lower one
    # no used pixel: both thresholds are +0.0 whatever the floor, and without a gate outlier the mask is empty
    empty = dict(fx, count=0)
    for floor in (0.0, 0.001):
        out = om.outliers(*pr.args_of(empty), fx["T0"], floor=floor)
        assert (out.code != 0).all() and not np.isin(out.code, (4, 5)).any()
        assert out.thresholds.tobytes() == np.zeros(2, F).tobytes() and not out.classes.any() and not out.mask.any()
    # a pixel the weights mask has code 6 and is never in the mask
    w = wr.block_mask((60, 80))
    T = np.asarray(fx["gt"], F)
    out = om.outliers(*pr.args_of(fx), T, w)
    assert np.isin(out.code[rr.BLOCK], (1, wr.MASKED)).all() and (out.code == wr.MASKED).sum() > 600
    assert not out.mask[rr.BLOCK].any()
    assert om.outliers(*pr.args_of(fx), T).mask[rr.BLOCK].sum() > 500            # ... which without the weights it is


# ------------------------------------------------------------------------------------------ what the mask is worth
KW = dict(huber_k=sr.K_HUBER)
BLOCK = np.zeros((60, 80), bool)
BLOCK[rr.BLOCK] = True
TABLE = {}


def table(scene, moved, stride, grow):
    """(errors in mm of the first solve, + 5 plain iterations, + 5 masked iterations; masked pixels in the block,
    outside it): frame 5 against frame 0's map, 10 huber_k = 1.345 iterations, the mask, 5 more from that pose"""
    key = (scene, moved, stride, grow)
    if key not in TABLE:
        fx = pr.convergence_fixture(scene=scene)
        fx = rr.moved_block(fx) if moved else fx
        floor = 0.0005 if (scene, moved) == ("facets", False) else 0.0
        T1, Tp, Tm, out = om.refine(fx, KW, stride, 10, 5, grow=grow, floor=floor)
        TABLE[key] = tuple(1e3 * rr.translation_error(T, fx["gt"]) for T in (T1, Tp, Tm)) + \
            (int(out.mask[BLOCK].sum()), int(out.mask[~BLOCK].sum()))
    return TABLE[key]


def row(scene, moved, stride, grow):
    e1, ep, em, inside, outside = table(scene, moved, stride, grow)
    return "| %s %s, %d | %d | %.3f | %.3f | %.3f | %d | %d |" % (scene, "moved" if moved else "clean", stride, grow, e1,
                                                                 ep, em, inside, outside)


ROWS = [(scene, moved, stride, grow) for scene in ("wave", "facets") for moved in (True, False) for stride in (1, 4)
        for grow in (0, 8)]


@pytest.mark.parametrize("scene,moved,stride,grow", ROWS)
def test_the_table_of_the_readme(scene, moved, stride, grow):
    """The README's table (section "Masking what moved"), every row to the digits of this restatement; translation error
    in mm, masked pixels of the block's 713 and of the 4 087 outside it.  facets clean runs with floor = 0.5 mm (its
    median is ~0); what that masks is recorded, not asserted."""
    line = row(scene, moved, stride, grow)
    print(line)
    assert line in open(os.path.join(REPO, "README.md")).read(), line
    e1, ep, em, inside, outside = table(scene, moved, stride, grow)
    if (scene, moved) == ("wave", True):
        assert em < e1 and em < ep                  # strictly closer than the first solve and than plain extra iterations
    if moved and grow == 0:                         # the mask itself, with the defaults
        assert inside >= 0.8 * BLOCK.sum() and outside <= 0.1 * (~BLOCK).sum(), (inside, outside)
    if (scene, moved) == ("wave", False):
        assert abs(em - e1) < 0.05 and abs(em - ep) < 0.05


# ------------------------------------------------------------------------------------------ the library
def test_new_symbols_are_declared_and_exported_at_abi_3():
    lib = _C.lib()
    assert set(NEW) <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
        assert not n.startswith("gs_projective_icp_")               # (that family is the route table's)
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3              # additions only: the ABI version stays
    assert C.sizeof(_C.PicpSeq) == 136
    # keys (H W uint32) | 2048 counters | the two thresholds, each part rounded up to 256 bytes
    assert lib.gs_picp_outlier_classes_scratch_bytes(48, 64) == 48 * 64 * 4 + 2048 * 4 + 256
    assert lib.gs_picp_outlier_classes_scratch_bytes(5, 7) == 256 + 2048 * 4 + 256
    assert lib.gs_picp_outlier_classes_scratch_bytes(0, 64) == 0 == lib.gs_picp_outlier_classes_scratch_bytes(1 << 16, 1 << 15)
    assert lib.gs_picp_outlier_classes_scratch_bytes(1 << 15, (1 << 16) - 1) > 0


def _seq(**kw):
    from tests.test_picp_color_cpu import _seq as color_seq
    return color_seq(**kw).base


ONE = (C.c_void_p * 1)(0xE00000)


def _classes(lib, q=None, weights=None, classes=ONE, th=None, B=1, H=48, W=64, dist_th=0.1, dot_th=0.866, hi=3.0, lo=1.5,
             floor=0.0):
    q = _seq() if q is None else q
    return lib.gs_picp_outlier_classes_batch_f32(C.pointer(q), weights, classes, th, B, H, W, dist_th, dot_th, hi, lo,
                                                 floor, None)


def _region(lib, classes=0x100000, depth=0x200000, mask=0x300000, B=1, H=48, W=64, min_support=6, grow=0, grow_depth=0.02):
    return lib.gs_region_mask_u8(classes, depth, mask, B, H, W, min_support, grow, grow_depth, None)


def test_every_entry_refuses_a_bad_descriptor_before_any_hip_call():
    """(fake pointers: a call that got past its checks would fault on this machine)"""
    lib = _C.lib()
    inf, nan = float("inf"), float("nan")
    bad = [(dict(classes=None), "bad arguments"), (dict(B=0), "bad arguments"), (dict(H=0), "bad arguments"),
           (dict(W=-1), "bad arguments"), (dict(H=1 << 16, W=1 << 15), "too large"), (dict(dist_th=nan), "NaN"),
           (dict(dot_th=nan), "NaN"), (dict(lo=0.0), "lo"), (dict(lo=nan), "lo"), (dict(lo=inf, hi=inf), "lo"),
           (dict(hi=1.0), "hi"), (dict(hi=inf), "hi"), (dict(hi=nan), "hi"), (dict(floor=-1e-3), "floor"),
           (dict(floor=nan), "floor"), (dict(floor=inf), "floor"),
           (dict(classes=(C.c_void_p * 1)(None)), "classes"), (dict(q=_seq(scratch=0xA00008)), "16-byte aligned")]
    bad += [(dict(q=_seq(**{k: 0})), "NULL") for k in ("vertex", "normal", "depth", "K16", "index", "model_pose16",
                                                       "init_pose16", "scratch", "points", "normals")]
    bad += [(dict(q=_seq(n_bound=-1)), "map size")]
    for kw, word in bad:
        assert _classes(lib, **kw) == 1, kw
        msg = lib.gs_last_error().decode()
        assert msg.startswith("gs_picp_outlier_classes_batch_f32") and word in msg, (kw, msg)
    assert lib.gs_last_error().decode() and _classes(lib, _seq(points=0, normals=0, n_bound=-1)) == 1
    bad = [(dict(classes=None), "NULL"), (dict(depth=None), "NULL"), (dict(mask=None), "NULL"), (dict(B=0), "bad arguments"),
           (dict(H=0), "bad arguments"), (dict(W=0), "bad arguments"), (dict(H=1 << 16, W=1 << 15), "too large"),
           (dict(min_support=0), "min_support"), (dict(min_support=10), "min_support"), (dict(grow=-1), "grow"),
           (dict(grow=17), "grow"), (dict(grow_depth=-1.0), "grow_depth"), (dict(grow_depth=nan), "grow_depth"),
           (dict(grow_depth=inf), "grow_depth")]
    for kw, word in bad:
        assert _region(lib, **kw) == 1, kw
        msg = lib.gs_last_error().decode()
        assert msg.startswith("gs_region_mask_u8") and word in msg, (kw, msg)


KERNELS = {"gs_picp_outlier_thresholds_kernel", "gs_picp_outlier_classes_kernel", "gs_weighted_picp_outlier_classes_kernel",
           "gs_region_mask_kernel"}


def test_kernels_use_no_scratch_spill_nothing_and_fit_the_lds():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp_outliers.hip", "gs_"],
                       capture_output=True, text=True, cwd=REPO, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if ln.strip() and not ln.startswith("#")}
    assert set(rows) == KERNELS, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        print(name, "VGPR", vgpr, "scratch", scratch, "occupancy", occ, "LDS", lds)
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
        assert int(lds) <= 64 * 1024, (name, lds)
    # the region pass: 66 x 66 cells of a float and three bytes
    assert int(rows["gs_region_mask_kernel"][6]) <= 66 * 66 * 7 + 64
    # the per-pixel kernels keep the 8 waves per SIMD of the linearise kernels they stand next to
    assert int(rows["gs_picp_outlier_classes_kernel"][3]) >= 8 and int(rows["gs_weighted_picp_outlier_classes_kernel"][3]) >= 8


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args():
    H, W = 4, 5
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]


def test_ops_check_their_arguments_and_have_no_cpu_fallback():
    from gradslam_amd import ops
    f = ops.projective_icp_outliers
    for kw in (dict(hi="3"), dict(lo=True), dict(floor=None), dict(min_support=6.0), dict(grow=True), dict(grow="1"),
               dict(grow_depth="x"), dict(return_classes=1), dict(return_thresholds=None), dict(dist_thresh="a")):
        with pytest.raises(TypeError, match=list(kw)[0]):
            f(*_cpu_args(), **kw)
    for kw in (dict(hi=1.0), dict(lo=0.0), dict(lo=-1.0), dict(hi=float("inf")), dict(lo=float("nan")), dict(floor=-0.1),
               dict(min_support=0), dict(min_support=10), dict(grow=-1), dict(grow=17), dict(grow_depth=-1.0),
               dict(grow_depth=float("nan")), dict(angle_thresh=91)):
        with pytest.raises(ValueError, match=list(kw)[0] if "hi" not in kw else "hi"):
            f(*_cpu_args(), **kw)
    with pytest.raises(TypeError, match="pixel_weights"):
        f(*_cpu_args(), pixel_weights=1.0)
    with pytest.raises(ValueError, match="pixel_weights"):
        f(*_cpu_args(), pixel_weights=torch.ones(5, 4))
    a = _cpu_args()
    with pytest.raises(TypeError, match="vertex"):
        f(None, *a[1:])
    with pytest.raises(ValueError, match="index"):
        f(*a[:4], a[4].int(), *a[5:])
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        f(*a)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        f(*a, pixel_weights=torch.ones(4, 5), grow=16, min_support=9, return_classes=True, return_thresholds=True)
    batch = [a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None], [(a[6], a[7], None, None)], a[8][None]]
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.projective_icp_outliers_batch(*batch)
    with pytest.raises(ValueError, match="one map per sequence"):
        ops.projective_icp_outliers_batch(*batch[:6], [], batch[7])
    cls, d = torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.ones(2, 3, 4, 5)
    for kw in (dict(min_support=0), dict(min_support=10), dict(grow=17), dict(grow=-1), dict(grow_depth=-1)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            ops.region_mask(cls, d, **kw)
    for kw in (dict(min_support=1.0), dict(grow=None), dict(grow_depth=None)):
        with pytest.raises(TypeError, match=list(kw)[0]):
            ops.region_mask(cls, d, **kw)
    with pytest.raises(TypeError, match="classes"):
        ops.region_mask(cls.int(), d)
    with pytest.raises(TypeError, match="depth"):
        ops.region_mask(cls, d.double())
    with pytest.raises(TypeError, match="classes"):
        ops.region_mask(None, d)
    for c2, d2 in ((cls, d[0]), (cls[0, 0, 0], d[0, 0, 0]), (cls[:, :, :0], d[:, :, :0])):
        with pytest.raises(ValueError, match="shape"):
            ops.region_mask(c2, d2)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.region_mask(cls, d, grow=16, min_support=1)
    assert ops.OutlierRule() == ops._outlier_rule("x") == (3.0, 1.5, 0.0, 6, 0, 0.02)
    assert ops._outlier_rule("x", **om.DEFAULTS) == ops.OutlierRule()


def test_provider_and_drivers_check_and_carry_the_rule():
    from gradslam_amd import ops
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider as Prov
    from gradslam_amd.slam import ICPSLAM, PointFusion
    p = Prov()
    assert p.outlier_mask is None and p.outlier_rule is None and p.last_outlier_mask is None
    assert p._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
    p = Prov(outlier_mask={})
    assert p.outlier_rule == ops.OutlierRule() and p.refine_iters == 5 and p.options.numiters == 10
    p = Prov(outlier_mask=dict(hi=4, lo=2, floor=0.001, min_support=4, grow=8, grow_depth=0.05, refine_iters=3),
             huber_k=1.345, differentiable=True, pixel_weights=lambda fr: None)
    assert p.outlier_rule == (4.0, 2.0, 0.001, 4, 8, 0.05) and p.refine_iters == 3 and p.differentiable
    assert Prov(outlier_mask=dict(grow=2), color_weight=0.2, color_huber_k=1.345).outlier_rule.grow == 2
    for bad in ("mask", 1, True, [("grow", 1)]):
        with pytest.raises(TypeError, match="outlier_mask"):
            Prov(outlier_mask=bad)
    with pytest.raises(TypeError, match="unknown keys"):
        Prov(outlier_mask=dict(grows=1))
    for kw, err in ((dict(refine_iters=0), ValueError), (dict(refine_iters=2.0), TypeError), (dict(refine_iters=True), TypeError),
                    (dict(hi=1.0), ValueError), (dict(lo=0), ValueError), (dict(grow=17), ValueError),
                    (dict(min_support=0), ValueError), (dict(grow_depth=-1), ValueError), (dict(floor="0"), TypeError)):
        with pytest.raises(err, match=list(kw)[0] if "hi" not in kw else "hi"):
            Prov(outlier_mask=kw)
    # the keyword is validated last: every refusal of today is the one raised, whatever the new keyword holds
    bad = "not a dict"
    for kw, err, word in ((dict(pixel_weights=1.0), TypeError, "pixel_weights"), (dict(differentiable=1), TypeError, "differentiable"),
                          (dict(deterministic_backward=1), TypeError, "deterministic_backward"),
                          (dict(stride=0), ValueError, "stride"), (dict(damp=0), ValueError, "damp"),
                          (dict(color_weight=-1), ValueError, "color_weight"),
                          (dict(color_weight=0.1, differentiable=True), ValueError, "differentiable"),
                          (dict(huber_delta=-1), ValueError, "huber_delta"),
                          (dict(color_huber_delta=0.1), ValueError, "color_huber_delta"),
                          (dict(huber_k=float("nan")), ValueError, "huber_k"),
                          (dict(color_huber_k=1.0), ValueError, "color_huber_k")):
        for om_kw in (bad, dict(grow=99), None):
            with pytest.raises(err, match=word) as e:
                Prov(outlier_mask=om_kw, **kw)
            assert "outlier_mask" not in str(e.value)
    f = lambda frames: None   # noqa: E731
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, odom_outlier_mask=dict(grow=3, refine_iters=2), huber_k=1.345,
                odom_pixel_weights=f)
        assert s.odomprov.outlier_rule.grow == 3 and s.odomprov.refine_iters == 2 and s.odomprov.pixel_weights is f
        assert cls(odom="projicp").odomprov.outlier_rule is None
        for odom in ("gt", "icp", "gradicp"):
            with pytest.raises(ValueError, match="odom_outlier_mask"):
                cls(odom=odom, odom_outlier_mask={})
            cls(odom=odom, odom_outlier_mask=None)
        with pytest.raises(TypeError, match="outlier_mask"):
            cls(odom="projicp", odom_outlier_mask=[1])
        with pytest.raises(ValueError, match="grow"):
            cls(odom="projicp", odom_outlier_mask=dict(grow=17))
        # today's refusals come first
        with pytest.raises(ValueError, match="odom_pixel_weights"):
            cls(odom="icp", odom_pixel_weights=f, odom_outlier_mask=bad)
        with pytest.raises(ValueError, match="huber_k"):
            cls(odom="icp", huber_k=1.0, odom_outlier_mask={})
        with pytest.raises(ValueError, match="differentiable"):
            cls(odom="projicp", color_weight=0.1, odom_differentiable=True, odom_outlier_mask=dict(grow=17))
    assert PointFusion(odom="projicp").fuse_outliers is True
    assert PointFusion(odom="projicp", odom_outlier_mask={}, fuse_outliers=False).fuse_outliers is False
    with pytest.raises(TypeError, match="fuse_outliers"):
        PointFusion(odom="projicp", odom_outlier_mask={}, fuse_outliers=0)
    with pytest.raises(ValueError, match="fuse_outliers"):
        PointFusion(odom="projicp", fuse_outliers=False)
    for odom in ("gt", "icp", "gradicp"):
        with pytest.raises(ValueError, match="fuse_outliers"):
            PointFusion(odom=odom, fuse_outliers=False)
        assert PointFusion(odom=odom, fuse_outliers=True).fuse_outliers


def test_masked_depth_is_a_copy_with_holes():
    from gradslam_amd.structures.rgbdimages import RGBDImages
    rng = np.random.default_rng(5)
    depth = torch.from_numpy(rng.uniform(0.5, 2.0, (2, 1, 6, 7, 1)).astype(np.float32))
    frames = RGBDImages(torch.zeros(2, 1, 6, 7, 3), depth.clone(), torch.eye(4).view(1, 1, 4, 4).repeat(2, 1, 1, 1),
                        torch.eye(4).view(1, 1, 4, 4).repeat(2, 1, 1, 1))
    mask = torch.from_numpy(rng.uniform(size=(2, 6, 7)) < 0.3)
    other = frames.masked_depth(mask)
    assert torch.equal(frames.depth_image, depth)                   # the caller's frame is untouched
    assert (other.depth_image[:, 0, ..., 0][mask] == 0).all() and torch.equal(other.depth_image[:, 0, ..., 0][~mask],
                                                                             depth[:, 0, ..., 0][~mask])
    assert other.poses is frames.poses and other.rgb_image is frames.rgb_image
    cf = frames.to_channels_first().masked_depth(mask.unsqueeze(1))
    assert cf.channels_first and torch.equal(cf.depth_image[:, 0, 0], other.depth_image[:, 0, ..., 0])
    with pytest.raises(TypeError):
        frames.masked_depth(mask.float())
    with pytest.raises(ValueError):
        frames.masked_depth(mask[:, :5])
