"""CPU tests of the joint projective ICP's colour Huber threshold from the colour residuals' median (color_huber_k): the
NumPy restatement (tests/picp_color_scale_ref.py) against itself and against the restatements it is built from, the
invariance under a change of the colours' units that a constant threshold does not have, what the rule buys on a scene
with a brightened patch (recorded, not tuned), the argument checks of the Python layers and the new C entry points."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import picp_color_ref as pcr
from tests import picp_color_scale_ref as csr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
K = csr.K_HUBER
WEIGHT = 0.2
NEW = ("gs_projective_icp_color_joint_scaled_scratch_bytes", "gs_projective_icp_color_joint_scaled_batch_f32",
       "gs_projective_icp_color_joint_scaled_rows_f32")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def terr(T, fx):
    return rr.translation_error(T, fx["gt"])


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("stride", [1, 3])
def test_the_threshold_is_the_constant_times_the_lower_median_of_a_sort(stride):
    fx = pcr.textured_fixture(scene="plane")
    q = csr.rows(*pcr.args_of(fx), fx["T0"], WEIGHT, color_huber_k=K, stride=stride)
    n = int(q.colored.sum())
    assert n > 100 and q.color_count == n and (q.r[~q.colored] == 0).all()
    med = np.sort(np.abs(q.r[q.colored]))[(n - 1) // 2]
    assert med > 0 and bits(q.cdelta) == bits(sr.constant(K) * med)
    # the colour weights are those of that threshold, the geometric ones are off
    assert np.array_equal(bits(q.color_weight), bits(rr.slot_weights(q.r, q.cdelta, q.colored)))
    assert (q.color_weight[q.colored] < 1).sum() > 10 and (q.color_weight[q.colored] == 1).sum() > 10
    assert np.array_equal(q.weight, (q.code == 0).astype(F)) and bits(q.delta) == bits(F(0))
    # r is the residual before the weight: bc = weight * r
    assert np.array_equal(bits(q.bc), bits(F(WEIGHT) * q.r))
    # the rows are picp_robust_ref's at that constant threshold
    const = rr.color_rows(*pcr.args_of(fx), fx["T0"], WEIGHT, 0.0, float(q.cdelta), stride=stride)
    assert np.array_equal(bits(const.sums), bits(q.sums))


def test_the_floor_rule():
    fx = pcr.textured_fixture(scene="plane")
    a = pcr.args_of(fx)
    free = csr.rows(*a, fx["T0"], WEIGHT, color_huber_k=K)
    low, high = float(free.cdelta) / 2, float(free.cdelta) * 2
    assert bits(csr.rows(*a, fx["T0"], WEIGHT, color_huber_k=K, color_huber_delta=low).cdelta) == bits(free.cdelta)
    assert bits(csr.rows(*a, fx["T0"], WEIGHT, color_huber_k=K, color_huber_delta=high).cdelta) == bits(F(high))
    # a product that is not above the floor, a NaN included, gives the floor
    r, on = np.array([np.nan, np.nan, 1.0], F), np.ones(3, bool)
    assert bits(csr.color_scale(r, on, K, 0.25)) == bits(F(0.25))
    assert bits(csr.color_scale(np.array([3.0, -1.0, 2.0, 9.0], F), np.ones(4, bool), K)) == bits(sr.constant(K) * F(2.0))
    # no coloured slot and a median of 0: the floor
    assert bits(csr.color_scale(r, np.zeros(3, bool), K, 0.125)) == bits(F(0.125))
    assert bits(csr.color_scale(np.array([0.0, 0.0, 5.0], F), on, K, 0.125)) == bits(F(0.125))
    assert bits(csr.color_scale(np.array([0.0, 0.0, 5.0], F), on, K)) == bits(F(0.0))
    # a view without any ok pixel: every iteration has the floor and the solve is the geometric one with its thresholds
    dark = dict(fx, model=np.zeros_like(fx["model"]))
    got = csr.color_solve(*pcr.args_of(dark), fx["T0"], WEIGHT, K, 0.0, K, 0.03, numiters=3)
    want = sr.color_solve(*pcr.args_of(dark), fx["T0"], WEIGHT, K, 0.0, 0.03, numiters=3)
    assert (got[1][:, 8] == 0).all() and np.array_equal(bits(got[3]), bits(np.full(3, 0.03, F)))
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("stride", [1, 4])
def test_without_the_constant_the_restatement_is_the_earlier_ones(stride):
    fx = rr.moved_block(pcr.textured_fixture(scene="plane"))
    a = pcr.args_of(fx)
    kw = dict(stride=stride, numiters=4)
    got = csr.color_solve(*a, fx["T0"], WEIGHT, K, 0.001, 0.0, 0.02, **kw)
    want = sr.color_solve(*a, fx["T0"], WEIGHT, K, 0.001, 0.02, **kw)
    for g, w_ in zip(got[:3], want):
        assert np.array_equal(bits(g), bits(w_))
    assert np.array_equal(bits(got[3]), bits(np.full(4, 0.02, F)))
    got = csr.color_solve(*a, fx["T0"], WEIGHT, 0.0, 0.005, 0.0, 0.02, **kw)
    want = rr.color_solve(*a, fx["T0"], WEIGHT, 0.005, 0.02, **kw)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[2]), bits(np.full(4, 0.005, F)))
    q = csr.rows(*a, fx["T0"], WEIGHT, 0.0, 0.005, 0.0, 0.02, stride=stride)
    r = rr.color_rows(*a, fx["T0"], WEIGHT, 0.005, 0.02, stride=stride)
    for name in r._fields:
        assert np.array_equal(np.asarray(getattr(q, name)), np.asarray(getattr(r, name))), name
    # and the rule changes the solve
    on = csr.color_solve(*a, fx["T0"], WEIGHT, 0.0, 0.005, K, 0.0, **kw)
    assert not np.array_equal(on[0], got[0]) and np.unique(on[3]).size > 1


# ------------------------------------------------------------------------------------------ 2. units
def test_a_change_of_the_colours_units_scales_the_threshold_and_keeps_the_solve():
    fx = pcr.textured_fixture(scene="plane")
    big = csr.scaled_colors(fx, 256.0)
    assert np.array_equal(bits(big["model"][..., :3]), bits(fx["model"][..., :3] * F(256)))
    kw = dict(stride=2, numiters=6)
    one = csr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, color_huber_k=K, **kw)
    two = csr.color_solve(*pcr.args_of(big), fx["T0"], WEIGHT / 256, color_huber_k=K, **kw)
    assert np.array_equal(bits(one[0]), bits(two[0])) and np.array_equal(bits(one[1]), bits(two[1]))
    assert (one[3] > 0).all() and np.array_equal(bits(two[3]), bits(one[3] * F(256)))
    q1 = csr.rows(*pcr.args_of(fx), fx["T0"], WEIGHT, color_huber_k=K, stride=2)
    q2 = csr.rows(*pcr.args_of(big), fx["T0"], WEIGHT / 256, color_huber_k=K, stride=2)
    assert np.array_equal(bits(q1.color_weight), bits(q2.color_weight)) and (q1.color_weight[q1.colored] < 1).any()
    # a constant threshold has a unit: the same number means something else in the other one
    c1 = rr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, 0.0, 0.02, **kw)
    c2 = rr.color_solve(*pcr.args_of(big), fx["T0"], WEIGHT / 256, 0.0, 0.02, **kw)
    assert not np.array_equal(bits(c1[0]), bits(c2[0]))


# ------------------------------------------------------------------------------------------ 5. what it buys
def test_what_the_estimated_colour_threshold_buys_on_a_brightened_patch():
    """The textured fronto-parallel plane at 60 x 80, frame 5 from pose 0 (25 mm off), color_weight 0.2, 12 iterations,
    stride 1; clean, and with the live COLOUR brightened by 0.35 in a block of 15 % of the image.  Translation error
    against the ground truth through the restatement, printed and recorded; the README table is this output.  The
    restatement's own numbers (mm), clean / brightened:
        unweighted                         1.721 / 53.119   (from 25.000: the patch drags the pose away)
        color_huber_delta = 0.02           1.720 /  4.106
        color_huber_k = 1.345              1.852 /  2.259
        color_huber_k = 1.345, 0 ... 255   1.852 /  2.259   (the same bits)
    Asserted: only the orderings the issue names -- on the brightened scene the estimated threshold ends closer to the
    ground truth than the unweighted solve, and the 0 ... 255 run equals the 0 ... 1 run."""
    clean = pcr.textured_fixture(scene="plane")
    scenes = {"clean": clean, "brightened": csr.brightened_block(clean)}
    kw = dict(stride=1, numiters=12)
    out = {}
    for name, fx in scenes.items():
        a = pcr.args_of(fx)
        big = csr.scaled_colors(fx, 256.0)
        runs = {"unweighted": pcr.solve(*a, fx["T0"], WEIGHT, **kw)[0],
                "color_huber_delta_0.02": rr.color_solve(*a, fx["T0"], WEIGHT, 0.0, 0.02, **kw)[0],
                "color_huber_k_1.345": csr.color_solve(*a, fx["T0"], WEIGHT, color_huber_k=K, **kw)[0],
                "color_huber_k_1.345_colours_0_255":
                    csr.color_solve(*pcr.args_of(big), fx["T0"], WEIGHT / 256, color_huber_k=K, **kw)[0]}
        out[name] = {k: terr(T, fx) for k, T in runs.items()}
        out[name]["start"] = terr(fx["T0"], fx)
        for k, v in out[name].items():
            print("%-10s %-36s %.3f mm" % (name, k, 1e3 * v))
        assert np.array_equal(bits(runs["color_huber_k_1.345"]), bits(runs["color_huber_k_1.345_colours_0_255"])), name
    rec_dir = os.environ.get("GRADSLAM_TEST_RECORD")
    if rec_dir:
        with open(os.path.join(rec_dir, "picp_color_scale_what_it_buys.json"), "w") as fh:
            json.dump(out, fh, indent=1)
    assert 0.024 < out["clean"]["start"] < 0.026
    assert out["brightened"]["color_huber_k_1.345"] < out["brightened"]["unweighted"]


# ------------------------------------------------------------------------------------------ 4. the library
def test_new_symbols_are_declared_and_exported_at_abi_3():
    lib = _C.lib()
    assert set(NEW) <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays
    size = lib.gs_projective_icp_color_joint_scaled_scratch_bytes
    for h, w, s in ((60, 80, 1), (37, 53, 3), (480, 640, 4)):
        ns = -(-h // s) * -(-w // s)
        old = lib.gs_projective_icp_color_scaled_scratch_bytes(h, w, s)
        # the colour-scaled scratch, then a second key table (nslots uint32), 2048 counters and a float, each aligned
        assert size(h, w, s) >= old + 4 * ns + 4 * 2048 + 4 and size(h, w, s) % 256 == 0
        assert size(h, w, s) - old == old - lib.gs_projective_icp_color_scratch_bytes(h, w, s)
    for bad in ((0, 64, 1), (48, 0, 1), (48, 64, 0), (-1, 64, 1), (1 << 16, 1 << 15, 1)):
        assert size(*bad) == 0, bad


def _seq(**kw):
    from tests.test_picp_color_cpu import _seq as color_seq
    return color_seq(**kw)


def _prm():
    return _C.PicpParams(4, 10, 1e-8, 0.1, 0.866)


def _calls(lib, q, prm):
    """the two new entries as functions of (huber_k, huber_floor, color_huber_k, color_huber_floor)"""
    return {
        "gs_projective_icp_color_joint_scaled_batch_f32":
            lambda k, fl, ck, cfl: lib.gs_projective_icp_color_joint_scaled_batch_f32(
                C.pointer(q), None, None, 1, 48, 64, prm, 0.1, k, fl, ck, cfl, None),
        "gs_projective_icp_color_joint_scaled_rows_f32":
            lambda k, fl, ck, cfl: lib.gs_projective_icp_color_joint_scaled_rows_f32(
                C.pointer(q), 48, 64, 4, 0.1, 0.866, 0.1, k, fl, ck, cfl, *([None] * 12), None, None, None),
    }


@pytest.mark.parametrize("bad", [float("nan"), -1e-3, float("inf"), -float("inf")])
def test_entry_points_reject_bad_constants_and_floors_before_any_hip_call(bad):
    lib = _C.lib()
    for name, call in _calls(lib, _seq(), _prm()).items():
        for args, word in (((K, 0.0, bad, 0.0), "color_huber_k"), ((K, 0.0, K, bad), "color_huber_floor"),
                           ((bad, 0.0, K, 0.0), "huber_k"), ((K, bad, K, 0.0), "huber_floor")):
            assert call(*args) == 1, (name, word)                 # GS_ERR_INVALID
            msg = lib.gs_last_error().decode()
            assert msg.startswith(name) and word in msg, msg


def test_entry_points_keep_the_checks_of_the_joint_solve():
    lib = _C.lib()
    prm = _prm()
    for name, call in _calls(lib, _seq(color=0), prm).items():    # a NULL colour pointer
        assert call(0.0, 0.0, K, 0.0) == 1, name
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "NULL" in msg and "color" in msg, msg
    for name, call in _calls(lib, _seq(scratch=0xA00008), prm).items():
        assert call(0.0, 0.0, K, 0.0) == 1, name
        msg = lib.gs_last_error().decode()
        assert msg.startswith(name) and "16-byte aligned" in msg, msg
    name = "gs_projective_icp_color_joint_scaled_batch_f32"
    batch = lib.gs_projective_icp_color_joint_scaled_batch_f32
    assert batch(None, None, None, 1, 48, 64, prm, 0.1, K, 0.0, K, 0.0, None) == 1
    assert batch(C.pointer(_seq()), None, None, 1, 48, 64, prm, -1.0, K, 0.0, K, 0.0, None) == 1
    assert lib.gs_last_error().decode().startswith(name) and "color_weight" in lib.gs_last_error().decode()
    assert batch(C.pointer(_seq()), None, None, 1, 48, 64, _C.PicpParams(0, 10, 1e-8, 0.1, 0.866), 0.1, K, 0.0, K, 0.0,
                 None) == 1
    assert "stride" in lib.gs_last_error().decode()
    null = (C.c_void_p * 1)(0)
    assert batch(C.pointer(_seq()), None, null, 1, 48, 64, prm, 0.1, 0.0, 0.0, K, 0.0, None) == 1
    assert "deltas" in lib.gs_last_error().decode()
    assert batch(C.pointer(_seq()), null, None, 1, 48, 64, prm, 0.1, K, 0.0, K, 0.0, None) == 1
    assert "deltas" in lib.gs_last_error().decode()


def test_the_rule_s_kernels_use_no_scratch_spill_nothing_and_keep_eight_waves():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp_scale.hip",
                        "gs_picp_scale_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_picp_scale_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_picp_scale_keys_kernel", "gs_picp_scale_color_keys_kernel", "gs_picp_scale_joint_keys_kernel",
                         "gs_picp_scale_select_kernel", "gs_picp_scale_clear_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
        assert int(occ) >= 8, (name, occ)
    # one first-digit histogram per residual asked for: 8 KB each, and nothing for the residual that is not
    one, two = 2048 * 4, 2 * 2048 * 4
    assert one <= int(rows["gs_picp_scale_keys_kernel"][6]) < one + 512
    assert one <= int(rows["gs_picp_scale_color_keys_kernel"][6]) < one + 512
    assert two <= int(rows["gs_picp_scale_joint_keys_kernel"][6]) < two + 512


# ------------------------------------------------------------------------------------------ 3. the Python layers
def _cpu_args():
    H, W = 4, 5
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4),
            torch.zeros(H, W, 3), torch.zeros(H, W, 4)]


def test_ops_check_color_huber_k():
    from gradslam_amd import ops
    a = _cpu_args()
    batch = lambda **kw: ops.projective_icp_color_batch(*[t[None] for t in a[:6]], [(a[6], a[7], None, None)],   # noqa: E731
                                                        a[8][None], a[9][None], a[10][None], **kw)
    for fn in (lambda **kw: ops.projective_icp_color(*a, **kw), lambda **kw: ops.projective_icp_color_rows(*a, **kw),
               batch):
        for bad in (float("nan"), -1e-3, float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="color_huber_k"):
                fn(color_weight=0.1, color_huber_k=bad)
        for bad in ("1.345", True, None):
            with pytest.raises(TypeError, match="color_huber_k"):
                fn(color_weight=0.1, color_huber_k=bad)
        with pytest.raises(ValueError, match="color_weight"):                    # nothing to estimate from
            fn(color_weight=0.0, color_huber_k=1.345)
        for good in (1.345, 2, 0, 0.0):                                          # a good value goes on to the call
            with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
                fn(color_weight=0.1, color_huber_k=good)
        with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
            fn(color_weight=0.1, color_huber_k=1.345, huber_k=1.345, huber_delta=1e-3, color_huber_delta=0.01)
        with pytest.raises(ValueError, match="huber_k"):
            fn(color_weight=0.1, color_huber_k=1.345, huber_k=-1.0)
    with pytest.raises(TypeError, match="huber_k"):                              # new to the rows call
        ops.projective_icp_color_rows(*a, color_weight=0.1, huber_k="1")
    for fn in (lambda **kw: ops.projective_icp_color(*a, **kw), batch):
        with pytest.raises(TypeError, match="return_color_scale"):
            fn(color_weight=0.1, return_color_scale=1)
        with pytest.raises(ValueError, match="differentiable"):                  # this refusal stays
            fn(color_weight=0.1, color_huber_k=1.345, differentiable=True)


def test_provider_and_drivers_check_and_carry_color_huber_k():
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    from gradslam_amd.slam import ICPSLAM, PointFusion
    prov = ProjectiveICPOdometryProvider(color_weight=0.2, color_huber_k=1.345, color_huber_delta=1e-3)
    assert (prov.color_huber_k, prov.color_huber_delta, prov.color_weight) == (1.345, 1e-3, 0.2)
    assert prov._kwargs() == dict(stride=1, numiters=10, damp=1e-8, dist_thresh=0.1, angle_thresh=30)   # five keys
    assert ProjectiveICPOdometryProvider().color_huber_k == 0.0
    assert ProjectiveICPOdometryProvider(color_weight=0.2, color_huber_k=2, huber_k=1.345).color_huber_k == 2
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="color_huber_k"):
            ProjectiveICPOdometryProvider(color_weight=0.2, color_huber_k=bad)
    for bad in ("1", True, None):
        with pytest.raises(TypeError, match="color_huber_k"):
            ProjectiveICPOdometryProvider(color_weight=0.2, color_huber_k=bad)
    with pytest.raises(ValueError, match="color_weight"):
        ProjectiveICPOdometryProvider(color_huber_k=1.345)
    with pytest.raises(ValueError, match="differentiable"):
        ProjectiveICPOdometryProvider(color_weight=0.2, color_huber_k=1.345, differentiable=True)
    for cls in (ICPSLAM, PointFusion):
        s = cls(odom="projicp", dsratio=2, color_weight=0.2, color_huber_k=1.345, color_huber_delta=1e-3)
        assert (s.color_huber_k, s.odomprov.color_huber_k, s.odomprov.color_huber_delta) == (1.345, 1.345, 1e-3)
        assert s.odomprov._kwargs() == dict(stride=2, numiters=20, damp=1e-8, dist_thresh=0.1, angle_thresh=30)
        assert cls(odom="projicp").odomprov.color_huber_k == 0.0
        for odom in ("gt", "icp", "gradicp"):
            with pytest.raises(ValueError, match="color_huber_k"):
                cls(odom=odom, color_huber_k=1.345)
            assert cls(odom=odom, color_huber_k=0.0).color_huber_k == 0.0
        with pytest.raises(ValueError, match="color_huber_k"):
            cls(odom="projicp", color_weight=0.2, color_huber_k=-1)
        with pytest.raises(TypeError, match="color_huber_k"):
            cls(odom="projicp", color_weight=0.2, color_huber_k="1")
        with pytest.raises(ValueError, match="color_weight"):
            cls(odom="projicp", color_huber_k=1.345)


def test_the_profile_tool_takes_the_constant():
    src = open(os.path.join(REPO, "tools", "projective_icp_profile.py")).read()
    assert "--color-huber-k" in src and "color_huber_k=args.color_huber_k" in src
