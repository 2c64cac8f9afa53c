"""CPU tests of surfel radii: the NumPy restatements (tests/radii_ref.py, tests/render_radii_ref.py) against the pinned
restatement of the constant-radius view (tests/render_ref.py), the table of the README, the layer rule over an oracle
frame loop, the committed float32 gaps of the backward cases, the host-side refusals and the kernels' resources."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import radii_ref
from tests import render_radii_backward_cases as cases
from tests import render_radii_ref as rrr
from tests import render_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = ("depth", "color", "normal", "confidence", "index", "keys")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def wave():
    s, m, lay = cases.scene("wave")
    return s, m, lay, s["intrinsics"][0].astype(np.float32)


# ------------------------------------------------------------------------------------------ the restatements
def test_sample_radius_by_hand():
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1] = 500.0, 540.0
    depth = np.array([[2.0, 0.0, 2.0, 2.0], [2.0, 2.0, -1.0, np.nan]], np.float32)
    n = np.zeros((2, 4, 3), np.float32)
    n[0, 0] = (0, 0, -1)            # fronto-parallel
    n[0, 1] = (0, 0, 1)             # no depth
    n[0, 2] = (0.8, 0, 0.6)         # oblique, under the cap
    n[0, 3] = (1, 0, 0)             # n_z = 0: the cap
    n[1, 0] = (0, 0, 0)             # no normal
    n[1, 1] = (0.9, 0.3, 0.1)       # grazing: the cap
    n[1, 2] = (0, 0, 1)
    n[1, 3] = (0, 0, 1)
    rho, valid = radii_ref.surfel_radius(depth, n, K)
    r0 = np.float32(np.float32(0.70710678) * np.float32(2.0)) / np.float32(520.0)
    assert valid.tolist() == [[True, False, True, True], [False, True, False, False]]
    want = [[r0, 0, r0 / np.float32(0.6), np.float32(2) * r0], [0, np.float32(2) * r0, 0, 0]]
    assert same_bits(rho, np.array(want, np.float32))
    assert rho.dtype == np.float32 and not np.signbit(rho).any()
    assert abs(float(r0) - 2.0 / 520 / np.sqrt(2)) < 1e-9


def test_splat_radius_by_hand():
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1] = 100.0, 100.0
    rho = np.array([0.0, -1.0, np.nan, np.inf, 0.0249, 0.025, 0.05, 1.0, 1e30], np.float32)
    z = np.full(len(rho), 2.0, np.float32)
    assert radii_ref.splat_radius(rho, K, z, 3).tolist() == [0, 0, 0, 0, 1, 1, 2, 3, 3]
    assert radii_ref.splat_radius(rho, K, z, 8).tolist() == [0, 0, 0, 0, 1, 1, 2, 8, 8]
    assert radii_ref.splat_radius(rho, K, z, 0).tolist() == [0] * 9


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("view", ["0", "o1", "z+0.4"])
def test_constant_r_is_the_constant_radius_view(k, view):
    """radii chosen so that the restatement itself reports r = k for every row in view: all five images and the key
    image are those of render_ref.render(radius=k)"""
    s, m, lay, K = wave()
    H, W = s["depths"].shape[1:3]
    pose = cases.view_pose(s, view)
    _, key = rr.row_keys(m.points, m.normals, m.ccounts, pose, K, H, W)
    z = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        radii = ((np.float32(k + 0.5) * z) / radii_ref.fbar_of(K)).astype(np.float32)
    for kw in ({}, {"min_confidence": float(np.median(m.ccounts))}):
        pix, _, r = rrr.row_splats(m.points, m.normals, m.ccounts, radii, pose, K, H, W, max_radius=3, **kw)
        assert (pix >= 0).sum() > 500 and (r[pix >= 0] == k).all(), "r = %d for every row in view" % k
        got, _ = rrr.render(m.points, m.normals, m.colors, m.ccounts, radii, pose, K, H, W, max_radius=3, **kw)
        want = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, radius=k, **kw)
        for name in IMAGES:
            assert same_bits(getattr(got, name), getattr(want, name)), (k, view, name)


def table():
    """dz -> dict(cov0, cov1, cov3, cov, fat1, fat3, fat) of the README's table, through the restatement"""
    s, m, lay, K = wave()
    H, W = s["depths"].shape[1:3]
    out = {}
    for dz in (0.0, 0.4, 1.0, -2.0):
        pose = rrr.moved(s["poses"][0], dz)
        d = {r: rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, radius=r).depth for r in (0, 1, 3)}
        own = rrr.render(m.points, m.normals, m.colors, m.ccounts, lay.radius, pose, K, H, W, max_radius=3)[0].depth
        out[dz] = dict(cov0=rrr.coverage(d[0]), cov1=rrr.coverage(d[1]), cov3=rrr.coverage(d[3]), cov=rrr.coverage(own),
                       fat1=rrr.fat_pixels(d[1], d[0]), fat3=rrr.fat_pixels(d[3], d[0]), fat=rrr.fat_pixels(own, d[0]))
    return out


def test_coverage_and_fat_pixels_of_the_table():
    t = table()
    for dz, row in t.items():
        print("dz %+.1f  coverage r=0 %.3f r=1 %.3f r=3 %.3f radii %.3f   fat r=1 %d r=3 %d radii %d"
              % (dz, row["cov0"], row["cov1"], row["cov3"], row["cov"], row["fat1"], row["fat3"], row["fat"]))
    assert t[1.0]["cov"] >= t[1.0]["cov1"] and t[1.0]["cov"] >= 4 * t[1.0]["cov0"]
    assert t[-2.0]["fat"] == 0 and t[-2.0]["fat1"] > 0
    assert round(t[0.0]["cov"], 3) == 1.000 and t[0.0]["fat"] < t[0.0]["fat1"]


def test_layer_rule_over_six_frames():
    """the restated layer against an independent float64 weighted mean per row; its weight is the confidence count"""
    from gradslam_amd.datasets.synthetic import make_sequence
    from oracle import oracle as o
    from tests import feature_fuse_ref as ffr
    s = make_sequence(6, 37, 53, seed=11)
    K = s["intrinsics"][0]
    H, W = 37, 53
    num, den, clean = np.zeros(6 * H * W), np.zeros(6 * H * W), np.ones(6 * H * W, bool)
    samples = np.zeros(6 * H * W, np.int64)
    seen = []

    def per_frame(f, m, lay):
        assert len(lay.radius) == len(lay.weight) == len(m)
        seen.append(len(m))

    m, lay = radii_ref.run_sequence(s["colors"], s["depths"], K, s["poses"], per_frame=per_frame)
    # the same samples, added up independently: replay the associations on the finished map's history
    from oracle import slam as oslam
    mm = oslam.MapState()
    import math
    for f in range(6):
        depth = s["depths"][f, ..., 0]
        v, n, a, _ = o.frame_maps(depth, K.astype(np.float32), 0.6)
        gv, gn = o.global_maps(v, n, depth, s["poses"][f])
        n_old = len(mm)
        best = np.full(H * W, -1, np.int32)
        if n_old:
            pix = o.project_map(mm.points, s["poses"][f], K.astype(np.float32), H, W)
            best, _ = o.associate(pix, mm.points, mm.normals, mm.ccounts, gv, gn, 0.05, math.cos(20 * math.pi / 180))
        mm.points, mm.normals, mm.colors, mm.ccounts = o.fuse_append(
            mm.points, mm.normals, mm.colors, mm.ccounts, best, gv, gn, s["colors"][f], a, depth, True)
        rows, n_new = ffr.rows_of_pixels(best, depth, n_old)
        assert n_new == len(mm) == seen[f]
        rho, valid = radii_ref.surfel_radius(depth, n, K)
        has = rows >= 0
        ok = has & valid.reshape(-1)
        np.add.at(num, rows[ok], a.reshape(-1)[ok].astype(np.float64) * rho.reshape(-1)[ok].astype(np.float64))
        np.add.at(den, rows[ok], a.reshape(-1)[ok].astype(np.float64))
        np.add.at(samples, rows[ok], 1)
        clean[rows[has & ~valid.reshape(-1)]] = False
    n = len(m)
    assert n == len(mm) and same_bits(m.points, mm.points) and same_bits(m.ccounts, mm.ccounts)
    fused = den[:n] > 0
    assert fused.mean() > 0.9 and (samples[:n] >= 4).sum() > 100, "rows with several samples"
    # at most 5 merges of 6 roundings each on positive terms, then one comparison in float64
    err = np.abs(lay.radius[fused] - num[:n][fused] / den[:n][fused]) / (num[:n][fused] / den[:n][fused])
    assert err.max() <= 5 * 6 * bc.EPS32, err.max()
    assert not lay.radius[~fused].any() and not lay.weight[~fused].any()
    c = clean[:n]
    assert c.mean() > 0.9 and same_bits(lay.weight[c], m.ccounts.reshape(-1)[c]), "the weight is the confidence count"
    assert (lay.weight[~c] < m.ccounts.reshape(-1)[~c]).all()
    cap = 2 * 0.70710678 * float(s["depths"].max()) / float(radii_ref.fbar_of(K))     # no sample exceeds the cap
    assert (lay.radius[fused] > 0).all() and lay.radius.max() <= cap * (1 + 1e-6)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_backward_cases_claims_and_committed_gaps(name):
    c = cases.build(name)
    cases.claims(c)
    for out, got, const in zip(cases.OUTPUTS, cases.gaps(name), cases.GAP[name]):
        print("%-12s %-11s gap %s committed %s" % (name, out, got, const))
        assert (got is None) == (const is None), (name, out)
        if const is None:
            continue
        if const == 0:
            assert got <= bc.EPS32, (name, out, got)
        else:
            assert const / bc.DRIFT <= got <= const * bc.DRIFT, (name, out, got, const)


# ------------------------------------------------------------------------------------------ the host side
def cpu_map(n=10):
    g = torch.Generator().manual_seed(0)
    P = torch.rand((n, 3), generator=g) + torch.tensor([0.0, 0.0, 1.0])
    return P, torch.zeros(n, 3), torch.rand((n, 3), generator=g), torch.ones(n, 1)


def test_refusals_of_ops_without_a_gpu():
    from gradslam_amd import _C, ops
    P, N, C, F = cpu_map()
    T, K = torch.eye(4).unsqueeze(0), torch.eye(4)
    rho = torch.full((10,), 0.01)
    call = lambda **kw: ops.render_map(P, N, C, F, T, K, 8, 8, **kw)       # noqa: E731
    with pytest.raises(ValueError, match="radius .1. must be 0 with radii"):
        call(radii=rho, radius=1)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="max_radius .* must be 0 ... 8"):
            call(radii=rho, max_radius=bad)
        with pytest.raises(ValueError, match="max_radius .* must be 0 ... 8"):
            call(max_radius=bad)
    with pytest.raises(TypeError, match="max_radius must be of type int"):
        call(radii=rho, max_radius=2.0)
    with pytest.raises(ValueError, match="radii.0. must be a float32 tensor"):
        call(radii=rho.double())
    for bad in (rho[:9], torch.cat([rho, rho[:1]]), rho.view(10, 1)):
        with pytest.raises(ValueError, match=r"radii.0. must have shape \(10,\)"):
            call(radii=bad)
    with pytest.raises(ValueError, match="one .N_b,. float32 tensor per sequence"):
        ops.render_map_batch([(P, N, C, F, None, None)], T.unsqueeze(0), K.unsqueeze(0), 8, 8, radii=[rho, rho])
    with pytest.raises(ValueError, match="one .N_b,. float32 tensor per sequence"):
        ops.render_map_batch([(P, N, C, F, None, None)], T.unsqueeze(0), K.unsqueeze(0), 8, 8, radii=rho)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        call(radii=rho)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        call(radii=rho, differentiable=True)
    idx = torch.zeros((1, 1, 8, 8), dtype=torch.int64)
    back = lambda **kw: ops.render_map_backward_batch([(P, N, None, None)], T.unsqueeze(0), K.unsqueeze(0), idx,   # noqa: E731
                                                      [torch.zeros(1, 1, 8, 8), None, None, None], 8, 8, **kw)
    with pytest.raises(ValueError, match="radius .2. must be 0 with radii"):
        back(radii=[rho], radius=2)
    with pytest.raises(ValueError, match=r"radii.0. must have shape \(10,\)"):
        back(radii=[rho[:3]])
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        back(radii=[rho])
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.surfel_radius(torch.ones(4, 5), torch.ones(4, 5, 3), torch.eye(4))
    with pytest.raises(ValueError, match="expected depth"):
        ops.surfel_radius(torch.ones(4, 5), torch.ones(4, 5, 2), torch.eye(4))
    with pytest.raises(ValueError, match="expected depth"):
        ops.surfel_radius(torch.ones(2, 4, 5), torch.ones(2, 4, 5, 3), torch.eye(4))


def test_refusals_of_the_containers_and_drivers():
    import gradslam_amd as gs
    P, N, C, F = cpu_map()
    K, T = torch.eye(4).view(1, 1, 4, 4), torch.eye(4).view(1, 1, 4, 4)
    pc = gs.Pointclouds(points=[P], normals=[N], colors=[C], features=[F])
    with pytest.raises(ValueError, match="radii='layer' needs a SurfelRadii layer"):
        pc.render(K, T, 8, 8, radii="layer")
    with pytest.raises(ValueError, match="radii must be None, 'layer' or a list"):
        pc.render(K, T, 8, 8, radii="map")
    pc.attach_features(gs.MapFeatures(1))
    with pytest.raises(ValueError, match="radii='layer' needs a SurfelRadii layer"):
        pc.render(K, T, 8, 8, radii="layer")             # (a user's one-channel layer is not the radii)
    with pytest.raises(ValueError, match="radius .2. must be 0 with radii"):
        pc.render(K, T, 8, 8, radii=[torch.ones(10)], radius=2)
    with pytest.raises(ValueError, match="max_radius .9. must be 0 ... 8"):
        pc.render(K, T, 8, 8, radii=[torch.ones(10)], max_radius=9)
    with pytest.raises(ValueError, match=r"radii.0. must have shape \(10,\)"):
        pc.render(K, T, 8, 8, radii=[torch.ones(11)])
    with pytest.raises(gs._C.HipExtensionError, match="no CPU fallback"):
        pc.render(K, T, 8, 8, radii=[torch.ones(10)])
    pc.detach_features()
    layer = gs.SurfelRadii()
    assert isinstance(layer, gs.MapFeatures) and layer.channels == 1 and layer.dtype == torch.float32
    pc.attach_features(layer)
    assert [tuple(t.shape) for t in layer.radii_list] == [(10,)] and not layer.radii_list[0].any()
    frame = gs.RGBDImages(torch.rand(1, 1, 8, 8, 3), torch.ones(1, 1, 8, 8, 1), K, T)
    slam = gs.slam.PointFusion(odom="gt")
    with pytest.raises(ValueError, match="the map's layer is a SurfelRadii"):
        slam.step(pc, frame, None, inplace=True, features=torch.zeros(1, 8, 8, 1))
    with pytest.raises(ValueError, match="the map's layer is a SurfelRadii"):
        slam.step(pc, frame, None, inplace=True, features_valid=torch.ones(1, 8, 8, dtype=torch.bool))
    bare = gs.Pointclouds(points=[P], normals=[N], colors=[C], features=[F])
    with pytest.raises(ValueError, match=r"attach_features\(gradslam_amd.SurfelRadii\(\)\)"):
        gs.slam.PointFusion(odom="gt", surfel_radii=True).step(bare, frame, None, inplace=True)
    with pytest.raises(ValueError, match="surfel_radii=True builds a map whose one layer is a SurfelRadii"):
        gs.slam.PointFusion(odom="gt", surfel_radii=True).forward(frame, features=torch.zeros(1, 1, 8, 8, 1))
    with pytest.raises(TypeError, match="surfel_radii must be of type bool"):
        gs.slam.PointFusion(surfel_radii=1)
    # the odometry
    with pytest.raises(ValueError, match="odom_surfel_radii is a switch of odom='projicp'"):
        gs.slam.PointFusion(odom="gradicp", odom_surfel_radii=True)
    with pytest.raises(ValueError, match="ICPSLAM.step is not supported on a map with a feature layer"):
        gs.slam.ICPSLAM(odom="projicp", odom_surfel_radii=True)
    with pytest.raises(TypeError, match="odom_surfel_radii must be of type bool"):
        gs.slam.PointFusion(odom="projicp", odom_surfel_radii="yes")
    prov = gs.slam.PointFusion(odom="projicp", odom_surfel_radii=True).odomprov
    assert prov.surfel_radii is True and prov.max_radius == 3 and prov.radius == 0
    assert gs.slam.PointFusion(odom="projicp").odomprov.surfel_radii is False
    Prov = gs.odometry.ProjectiveICPOdometryProvider
    with pytest.raises(ValueError, match="radius .1. must be 0 with surfel_radii"):
        Prov(radius=1, surfel_radii=True)
    with pytest.raises(ValueError, match="max_radius .9. must be 0 ... 8"):
        Prov(max_radius=9)
    with pytest.raises(ValueError, match="surfel_radii needs a SurfelRadii layer on the map"):
        Prov(surfel_radii=True, max_radius=8).localize(bare, frame, T)


def test_c_entries_check_their_arguments_without_a_gpu():
    from gradslam_amd import _C
    lib = _C.lib()
    assert {"gs_surfel_radius_f32", "gs_render_map_radii_dc_f32", "gs_render_map_radii_backward_dc_f32"} <= set(_C.EXPORTS)
    assert not any("radii" in n and n.endswith("_scratch_bytes") for n in _C.EXPORTS), "no new scratch sizer"
    import ctypes
    seqs = (_C.RenderSeq * 1)()
    none = (ctypes.c_void_p * 1)()
    assert lib.gs_render_map_radii_dc_f32(seqs, None, 1, 1, 4, 4, 3, 0.0, 0, None) == 1
    assert b"gs_render_map_radii_dc_f32" in lib.gs_last_error() and b"radii" in lib.gs_last_error()
    for cap in (-1, 9):
        assert lib.gs_render_map_radii_dc_f32(seqs, none, 1, 1, 4, 4, cap, 0.0, 0, None) == 1
        assert b"max_radius must be 0 ... 8" in lib.gs_last_error()
    assert lib.gs_render_map_radii_dc_f32(seqs, none, 1, 1, 4, 4, 8, 0.0, 0, None) == 1      # poses / K / scratch are NULL
    assert b"NULL pointer" in lib.gs_last_error()
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 4, 0.0, 0, None) == 1
    assert b"gs_render_map_dc_f32: radius must be 0, 1, 2 or 3" in lib.gs_last_error()
    bseqs = (_C.RenderBackwardSeq * 1)()
    assert lib.gs_render_map_radii_backward_dc_f32(bseqs, None, 1, 1, 4, 4, 3, None) == 1
    assert b"gs_render_map_radii_backward_dc_f32" in lib.gs_last_error()
    assert lib.gs_render_map_radii_backward_dc_f32(bseqs, none, 1, 1, 4, 4, 9, None) == 1
    assert b"max_radius must be 0 ... 8" in lib.gs_last_error()
    assert lib.gs_render_map_backward_dc_f32(bseqs, 1, 1, 4, 4, 4, None) == 1
    assert b"gs_render_map_backward_dc_f32: radius must be 0, 1, 2 or 3" in lib.gs_last_error()
    assert lib.gs_surfel_radius_f32(None, 0, None, 0, None, 1, 4, 4, None, None, None) == 1
    assert b"gs_surfel_radius_f32: NULL pointer" in lib.gs_last_error()
    assert lib.gs_surfel_radius_f32(None, 0, None, 0, None, 1, 0, 4, None, None, None) == 1
    assert lib.gs_surfel_radius_f32(None, 0, None, 0, None, 0, 4, 4, None, None, None) == 0   # nothing to do


def test_radii_kernels_use_no_scratch_and_spill_nothing():
    """The key pass with radii keeps the occupancy of the plain one (<= 64 VGPRs, 8 waves per SIMD), the row pass of the
    backward that of its plain twin; nothing spills, nothing uses scratch."""
    rows = {}
    for src, pat in (("gs_render.hip", "gs_rview_"), ("gs_radii.hip", "gs_surfel_radius")):
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), src, pat],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        print(r.stdout)
        rows.update({ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
                     if pat in ln and not ln.startswith("#")})
    assert {"gs_rview_radii_key_kernel", "gs_rview_radii_backward_rows_kernel", "gs_rview_backward_rows_kernel",
            "gs_surfel_radius_kernel"} <= set(rows), rows
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
    assert int(rows["gs_rview_radii_key_kernel"][0]) <= 64 and int(rows["gs_rview_radii_key_kernel"][3]) >= 8
    assert int(rows["gs_surfel_radius_kernel"][3]) >= 8
    assert int(rows["gs_rview_radii_backward_rows_kernel"][3]) >= int(rows["gs_rview_backward_rows_kernel"][3])
