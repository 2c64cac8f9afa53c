"""CPU-only tests of the model view: argument validation of the C entry points (GS_ERR_INVALID before any HIP call), the
"no CPU fallback" error of the Python layer, the sanity of the NumPy restatement the GPU tests compare against
(tests/render_ref.py), and the register allocation of the two kernels (hipcc cross-compiles and reports it)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from gradslam_amd.datasets.synthetic import make_sequence
from oracle import oracle as o
from oracle import slam as oslam
from tests import render_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _C.lib()
    assert lib.gs_render_scratch_bytes(1, 480, 640) >= 8 * 480 * 640
    assert lib.gs_render_scratch_bytes(3, 480, 640) >= 3 * 8 * 480 * 640
    # views beyond one launch reuse the key images of the first
    assert lib.gs_render_scratch_bytes(64, 480, 640) == lib.gs_render_scratch_bytes(4, 480, 640)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 16)):
        assert lib.gs_render_scratch_bytes(*bad) == 0, bad
    assert lib.gs_render_map_dc_f32(None, 1, 1, 4, 4, 0, 0.0, 0, None) == 1
    assert b"gs_render_map_dc_f32" in lib.gs_last_error()
    seqs = (_C.RenderSeq * 1)()
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 0, None) == 1     # poses / K / scratch are NULL
    assert b"NULL" in lib.gs_last_error()
    fake = C.c_void_p(4096)   # never dereferenced: every call below fails its checks first
    seqs[0].poses16 = seqs[0].K16 = seqs[0].scratch = fake
    for args in ((0, 1, 4, 4, 0, 0.0, 0), (1, 0, 4, 4, 0, 0.0, 0), (1, 1, 0, 4, 0, 0.0, 0), (1, 1, 4, -4, 0, 0.0, 0),
                 (1, 1, 1 << 16, 1 << 16, 0, 0.0, 0), (1, 1, 4, 4, 4, 0.0, 0), (1, 1, 4, 4, -1, 0.0, 0),
                 (1, 1, 4, 4, 0, float("nan"), 0)):
        assert lib.gs_render_map_dc_f32(seqs, *args, None) == 1, args
    seqs[0].map.n_bound = 1 << 32
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 0, None) == 1
    assert b"2^32" in lib.gs_last_error()
    seqs[0].map.n_bound = -1
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 0, None) == 1
    seqs[0].map.n_bound = 10                                                     # rows but no points
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 0, None) == 1
    assert b"points" in lib.gs_last_error()
    seqs[0].map.points = fake
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 1, None) == 1     # cull_backfaces without normals
    assert b"normals" in lib.gs_last_error()
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.5, 0, None) == 1     # min_confidence without counts
    assert b"ccounts" in lib.gs_last_error()
    seqs[0].color = fake
    assert lib.gs_render_map_dc_f32(seqs, 1, 1, 4, 4, 0, 0.0, 0, None) == 1     # a colour image without colours
    assert b"colors" in lib.gs_last_error()


def test_cpu_tensors_are_rejected_loudly():
    import gradslam_amd as gs
    from gradslam_amd import ops
    from gradslam_amd.metrics import depth_residual
    p = torch.rand(5, 3)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.render_map(p, p, p, torch.rand(5, 1), torch.eye(4), torch.eye(4), 4, 4)
    pc = gs.Pointclouds(points=[p], normals=[p], colors=[p], features=[torch.rand(5, 1)])
    K, poses = torch.eye(4).reshape(1, 1, 4, 4), torch.eye(4).reshape(1, 1, 4, 4)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        pc.render(K, poses, 4, 4)
    frames = gs.RGBDImages(torch.rand(1, 1, 4, 4, 3), torch.rand(1, 1, 4, 4, 1), K, poses)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        depth_residual(pc, frames)


def test_render_argument_checks_of_the_container():
    import gradslam_amd as gs
    p = torch.rand(5, 3)
    K, poses = torch.eye(4).reshape(1, 1, 4, 4), torch.eye(4).reshape(1, 1, 4, 4)
    with pytest.raises(ValueError, match="empty pointclouds"):
        gs.Pointclouds().render(K, poses, 4, 4)
    with pytest.raises(ValueError, match="surfel map"):
        gs.Pointclouds(points=[p]).render(K, poses, 4, 4)
    pc = gs.Pointclouds(points=[p], normals=[p], colors=[p], features=[torch.rand(5, 1)])
    with pytest.raises(TypeError, match="Expected poses to be of type tensor"):
        pc.render(K, None, 4, 4)
    with pytest.raises(ValueError, match="poses should have shape"):
        pc.render(K, torch.eye(4), 4, 4)
    with pytest.raises(ValueError, match="intrinsics should have shape"):
        pc.render(torch.eye(4), poses, 4, 4)


@pytest.fixture(scope="module")
def small():
    s = make_sequence(6, 96, 128, seed=0)
    m, _ = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], s["poses"], odom="gt")
    return s, m


def test_restatement_every_competing_row_meets_a_key_not_above_its_own(small):
    s, m = small
    H, W, K = 96, 128, s["intrinsics"][0]
    assert len(m) == 20410
    for f, radius in ((0, 0), (3, 0), (5, 1)):
        pose = s["poses"][f]
        r = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, radius=radius)
        pix, key = rr.row_keys(m.points, m.normals, m.ccounts, pose, K, H, W)
        inside = pix >= 0
        assert inside.sum() > 0.5 * len(m)
        assert (r.keys[pix[inside]] <= key[inside]).all()
        # every winner is a row that competes, its pixel within `radius` of the winner's own, and holds its depth
        hit = r.index >= 0
        rows = r.index[hit]
        assert inside[rows].all()
        hh, ww = np.nonzero(hit)
        assert (np.abs(pix[rows] // W - hh) <= radius).all() and (np.abs(pix[rows] % W - ww) <= radius).all()
        Tinv, _ = rr.camera_inverse(pose)
        assert np.array_equal(o.transform_points(m.points, Tinv)[rows, 2], r.depth[hit][:, 0])
        assert (r.depth[hit] > 0).all() and not r.depth[~hit].any() and not r.color[~hit].any()
        st = rr.residual_stats(r.depth, s["depths"][f])
        # (radius 0: a pixel shows a surfel of its own; a wider splat shows the nearest surfel of the neighbourhood)
        assert st["coverage"] > 0.98 and (radius > 0 or st["median_abs"] < 2e-3), st
    # the camera matrix of the restatement inverts the pose
    Tinv, Trot = rr.camera_inverse(s["poses"][4])
    assert np.abs(Tinv.astype(np.float64) @ s["poses"][4].astype(np.float64) - np.eye(4)).max() < 1e-6
    assert not Trot[:3, 3].any()


def test_restatement_duplicated_rows_pick_the_lower_index(small):
    s, m = small
    H, W, K, pose = 96, 128, s["intrinsics"][0], s["poses"][2]
    n = len(m)
    base = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W)
    twice = rr.render(*[np.concatenate([a, a]) for a in (m.points, m.normals, m.colors, m.ccounts)], pose, K, H, W)
    assert np.array_equal(twice.index, base.index) and twice.index.max() < n
    assert np.array_equal(twice.depth, base.depth)
    # filters only ever remove competitors
    cc = np.sort(m.ccounts.reshape(-1))
    for kw in ({"min_confidence": float(cc[len(cc) // 2])}, {"cull_backfaces": True}):
        f = rr.render(m.points, m.normals, m.colors, m.ccounts, pose, K, H, W, **kw)
        assert (f.keys >= base.keys).all() and (f.keys > base.keys).any()


def test_render_kernels_use_no_scratch_and_spill_nothing():
    """Both passes are memory-bound streams over the map / the image: a spill would add private-segment traffic to every
    row, and 8 waves per SIMD keep enough loads and atomics in flight (<= 64 VGPRs)."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_render.hip", "gs_render_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines() if "gs_render_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_render_key_kernel", "gs_render_resolve_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
        assert int(vgpr) <= 64 and int(occ) >= 8, (name, vgpr, occ)
