"""The one-call step without the outputs nothing in the frame loop reads: gs_step_seq::vertex / alpha NULL (the local
vertex of a pixel is fm_vertex of its depth wherever the step uses it), best_pix NULL (the tie-marker table lives in the
update's scratch and the winners do not write it).  Everything here is bit for bit: the same poses, map rows and counts
with and without the outputs, against the generic path (the separate association kernels: the independent statement of
what the implicit vertex must reproduce), with ties in every pixel, and the refusals of the half-given combinations."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from tests import scratch_guard

pytestmark = pytest.mark.gpu

DIST_TH, DOT_TH, SIGMA, DS = 0.05, math.cos(20 * math.pi / 180), 0.6, 4
T = torch.from_numpy
ATTRS = ("points_list", "normals_list", "colors_list", "features_list")


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


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


# ------------------------------------------------------------------------ 1: with and without the outputs
def test_same_bits_with_and_without_the_local_maps(gs, monkeypatch):
    """B = 2, 67 x 131 (no multiple of the 64 x 8 frame-map tile nor of ds = 4), 5 frames with the generator's 5 % holes:
    the step that writes no vertex / alpha map gives the poses and the map of the step that does, and the container
    computes the maps it was not handed -- local vertex, alpha, global vertex -- to the same bits when asked."""
    from gradslam_amd.slam import _fastpath
    B, L, H, W = 2, 5, 67, 131
    seqs = [make_sequence(L, H, W, seed=61 + b) for b in range(B)]
    stack = lambda k: T(np.stack([s[k] for s in seqs])).cuda()  # noqa: E731

    def run(materialise):
        monkeypatch.setattr(_fastpath, "STEP_LOCAL_MAPS", materialise)
        poses = stack("poses")
        poses[:, 1:] = poses[:, :1]
        frames = gs.RGBDImages(stack("colors"), stack("depths"), stack("intrinsics"), poses)
        slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
        pc, prev, rec, fast = gs.Pointclouds(device="cuda"), None, [], 0
        for i in range(L):
            live = frames[:, i]
            pc, p = slam.step(pc, live, prev, inplace=True)
            if i >= 2:   # (frame 0 has no previous frame, frame 1 finds the counts not yet grouped: generic path)
                assert (live._vertex_map is not None) == materialise, i
                assert (live._alpha_cache is not None) == materialise, i
                fast += 1
            rec += [host(p[:, 0]), host(live.vertex_map), host(live._alpha_map(SIGMA)), host(live.global_vertex_map)]
            prev = live
        assert fast == L - 2
        n = [int(x.shape[0]) for x in pc.points_list]
        return rec + [np.concatenate([host(x) for x in getattr(pc, k)]) for k in ATTRS] + [np.array(n, np.float32)]

    a, b = run(True), run(False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), i


# ------------------------------------------------------------------------ 2: fast path against the generic path
_AB_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from gradslam_amd.datasets.synthetic import make_sequence
B, L, H, W = 2, 5, 67, 131
seqs = [make_sequence(L, H, W, seed=71 + b) for b in range(B)]
d0, d1 = seqs[0]["depths"], seqs[1]["depths"]
# sequence 0: last row and last column valid (the forward-difference normal's edge rule sees no hole there)
fill = np.float32(d0[d0 > 0].mean())
d0[:, -1, :, :] = np.where(d0[:, -1, :, :] > 0, d0[:, -1, :, :], fill)
d0[:, :, -1, :] = np.where(d0[:, :, -1, :] > 0, d0[:, :, -1, :], fill)
assert (d0[:, -1] > 0).all() and (d0[:, :, -1] > 0).all()
# sequence 1: first row all holes (zero vertices at the border)
d1[:, 0, :, :] = 0.0
st = lambda k: torch.from_numpy(np.stack([s[k] for s in seqs])).cuda()
poses = st("poses"); poses[:, 1:] = poses[:, :1]
frames = gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)
slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
pc, prev, rec, implicit = gs.Pointclouds(device="cuda"), None, [], 0
for i in range(L):
    live = frames[:, i]
    pc, p = slam.step(pc, live, prev, inplace=True)
    implicit += int(live._vertex_map is None)
    prev = live
    rec.append(p[:, 0].cpu().numpy())
cat = lambda xs: np.concatenate([x.cpu().numpy() for x in xs])
np.savez(sys.argv[1], poses=np.stack(rec), n=np.array([int(x.shape[0]) for x in pc.points_list]), implicit=implicit,
         pts=cat(pc.points_list), nrm=cat(pc.normals_list), col=cat(pc.colors_list), cc=cat(pc.features_list))
"""


def test_fast_path_without_the_outputs_equals_generic_path(tmp_path):
    """The default fast path (no vertex map, no alpha map, no correspondence table) against GRADSLAM_HIP_FASTPATH=0, which
    makes the maps with the frame-map kernel and associates through the separate kernels: the same poses, points, normals,
    colours, confidence counts and row counts."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fast in ("1", "0"):
        out = str(tmp_path / ("fast%s.npz" % fast))
        env = dict(os.environ, GRADSLAM_HIP_FASTPATH=fast)
        for k in ("GRADSLAM_HIP_STEP_LOCAL_MAPS", "GRADSLAM_HIP_STEP_GLOBAL_MAPS", "GRADSLAM_HIP_STEP_BEST_PIX"):
            env.pop(k, None)
        subprocess.run([sys.executable, "-c", _AB_SCRIPT % repo, out], check=True, timeout=600, env=env)
        outs.append(np.load(out))
    a, b = outs
    assert int(a["implicit"]) == 3, "frames 2..4 must have taken the fast path without a vertex map"
    for k in ("poses", "pts", "nrm", "col", "cc"):
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["n"], b["n"])


# ------------------------------------------------------------------------ 3: ties without the table
def _build_maps(ops, seeds, H, W, frames=2):
    """per sequence: a surfel map of `frames` fused frames on capacity-backed buffers + the next frame's inputs"""
    out = []
    for seed in seeds:
        s = make_sequence(frames + 1, H, W, seed=seed, hole_frac=0.05 + 0.03 * (seed % 3))
        K = dev(s["intrinsics"][0])
        cap = (frames + 2) * H * W
        bufs = [torch.zeros((cap, k), device="cuda") for k in (3, 3, 3, 1)]
        n_map = 0
        for f in range(frames):
            d, pose = dev(s["depths"][f, ..., 0]), dev(s["poses"][f])
            v, n, a, _ = ops.frame_maps(d, K, SIGMA)
            gv, gn = ops.global_maps(v, n, d, pose)
            pix = ops.project_map(bufs[0][:n_map], pose, K, H, W)
            best = ops.associate(pix, bufs[0][:n_map], bufs[1][:n_map], bufs[3][:n_map], gv, gn, DIST_TH, DOT_TH)
            n_map = ops.fuse_append_(*bufs, n_map, best, gv, gn, dev(s["colors"][f]), a, d)
        out.append(dict(seq=s, K=K, bufs=bufs, n=n_map))
    return out


@pytest.fixture(scope="module")
def duplicated(ops):
    """maps in which every row has an exact duplicate with a higher index (two in the third sequence), the next frame of
    each, and what the table-level kernels make of them -- computed once, never written to"""
    H, W = 120, 160
    maps = _build_maps(ops, (5, 6, 7), H, W)
    for i, m in enumerate(maps):
        n, reps = m["n"], (3 if i == 2 else 2)
        big = [torch.zeros((reps * n + 2 * H * W, t.shape[1]), device="cuda") for t in m["bufs"]]
        for t, src in zip(big, m["bufs"]):
            for r in range(reps):
                t[r * n:(r + 1) * n] = src[:n]
        m["bufs"], m["n"], m["first"] = big, reps * n, n
    ref, frames = [], []
    for m in maps:
        s = m["seq"]
        d, pose = dev(s["depths"][2, ..., 0]), dev(s["poses"][2])
        v, n, a, _ = ops.frame_maps(d, m["K"], SIGMA)
        gv, gn = ops.global_maps(v, n, d, pose)
        bufs = [t.clone() for t in m["bufs"]]
        pix = ops.project_map(bufs[0][:m["n"]], pose, m["K"], H, W)
        best = ops.associate(pix, bufs[0][:m["n"]], bufs[1][:m["n"]], bufs[3][:m["n"]], gv, gn, DIST_TH, DOT_TH)
        n1 = ops.fuse_append_(*bufs, m["n"], best, gv, gn, dev(s["colors"][2]), a, d)
        ref.append((bufs, n1, best))
        frames.append((v, n, d, dev(s["colors"][2]), a, pose))
    return dict(H=H, W=W, maps=maps, ref=ref, frames=frames)


def test_ties_settle_the_same_without_the_table(ops, duplicated):
    H, W, maps, ref, frames = (duplicated[k] for k in ("H", "W", "maps", "ref", "frames"))
    st = lambda i: torch.stack([f[i] for f in frames])  # noqa: E731
    K = torch.stack([m["K"] for m in maps])
    runs = []
    for want in (True, False):
        mv = [(*[t.clone() for t in m["bufs"]], m["n"], None) for m in maps]
        cnt, _, _, best = ops.update_map_fusion_batch_(mv, st(0), st(1), st(2), st(3), st(4), st(5), K, DIST_TH, DOT_TH,
                                                       want_best_pix=want)
        assert (best is not None) == want
        runs.append((mv, host(cnt), best))
    (mv_a, cnt_a, best_a), (mv_b, cnt_b, _) = runs
    assert np.array_equal(cnt_a, cnt_b)
    for b, m in enumerate(maps):
        bufs, n1, rbest = ref[b]
        assert cnt_a[b] == n1
        # ties really occurred: every winner is a row of the first copy although a later copy holds the same key
        assert int((rbest >= 0).sum()) > 1000 and int(rbest.max()) < m["first"]
        assert torch.equal(best_a[b], rbest), b           # the requested table is the table-level kernels'
        for k in range(4):
            assert torch.equal(mv_a[b][k][:n1], bufs[k][:n1]), (b, k)
            assert torch.equal(mv_b[b][k], mv_a[b][k]), (b, k)   # (the whole buffer: nothing behind the count either)


def _step_call(ops, duplicated, outputs, spoil=None):
    """gs_pointfusion_step_batch_f32 on the duplicated maps and their next frames, numiters = 0 (out_pose = prev_pose = the
    frame's pose).  outputs: vertex / alpha / best_pix given (True) or NULL.  spoil(seqs, tensors): edits the descriptors
    before the call.  Returns (status, poses, counts, buffers)."""
    from gradslam_amd import _C
    L = _C.lib()
    H, W, maps, frames = (duplicated[k] for k in ("H", "W", "maps", "frames"))
    B, P, f32 = len(maps), H * W, torch.float32
    depth, rgb = torch.stack([f[2] for f in frames]), torch.stack([f[3] for f in frames])
    prev, K = torch.stack([f[5] for f in frames]).contiguous(), torch.stack([m["K"] for m in maps]).contiguous()
    vertex, normal = torch.empty((B, H, W, 3), dtype=f32, device="cuda"), torch.empty((B, H, W, 3), dtype=f32, device="cuda")
    alpha, out_pose = torch.empty((B, H, W), dtype=f32, device="cuda"), torch.zeros((B, 4, 4), dtype=f32, device="cuda")
    best = torch.empty((B, P), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int64, device="cuda")
    stores = [[t.clone() for t in m["bufs"]] for m in maps]
    n_dev = dev(np.array([m["n"] for m in maps], np.int64))
    seqs = (_C.StepSeq * B)()
    guards = scratch_guard.GuardLog(0xFF)
    for b, (m, bufs) in enumerate(zip(maps, stores)):
        cap = int(bufs[0].shape[0])
        # exactly what the sizers say, between guard bands, poisoned with 0xFF (tests/scratch_guard.py)
        loc = scratch_guard.guarded_buffer(guards, "loc_scratch%d" % b, L.gs_localize_scratch_bytes(H, W, DS, cap), "cuda")
        upd = scratch_guard.guarded_buffer(guards, "upd_scratch%d" % b, L.gs_update_map_scratch_bytes(cap, H, W), "cuda")
        q = seqs[b]
        q.depth, q.rgb, q.K16 = depth[b].data_ptr(), rgb[b].data_ptr(), K[b].data_ptr()
        q.prev_pose16, q.out_pose16 = prev[b].data_ptr(), out_pose[b].data_ptr()
        q.normal = normal[b].data_ptr()
        q.vertex, q.alpha = (vertex[b].data_ptr(), alpha[b].data_ptr()) if outputs else (None, None)
        q.gvertex = q.gnormal = None
        q.best_pix, q.new_count_out = (best[b].data_ptr() if outputs else None), cnt[b:].data_ptr()
        q.map = _C.MapView(*[t.data_ptr() for t in bufs], cap, int(m["n"]), n_dev[b:].data_ptr())
        q.loc_scratch, q.upd_scratch = loc.data_ptr(), upd.data_ptr()
    if spoil is not None:
        spoil(seqs, dict(vertex=vertex, alpha=alpha, best=best))
    prm = _C.IcpParams(1, 0, 1e-8, -1.0, 2.0, 1.0, 1.0, 200.0)
    status = L.gs_pointfusion_step_batch_f32(seqs, B, H, W, DS, prm, ops.two_sigma_sq(SIGMA), DIST_TH, DOT_TH, 1,
                                             _C.stream(depth.device))
    torch.cuda.synchronize()
    ok, hits = scratch_guard.intact(guards)
    assert ok, ("the step wrote outside a scratch of exactly the sizer's size", hits)
    return status, host(out_pose), host(cnt), [[host(t) for t in bufs] for bufs in stores]


def test_step_with_ties_gives_the_same_bits_without_its_outputs(ops, duplicated):
    """the same duplicated maps one step through gs_pointfusion_step_batch_f32: vertex, alpha and best_pix all NULL against
    all three given -- pose, every buffer (rows behind the count included) and the counts"""
    sa, pose_a, cnt_a, bufs_a = _step_call(ops, duplicated, True)
    sb, pose_b, cnt_b, bufs_b = _step_call(ops, duplicated, False)
    assert sa == 0 and sb == 0
    assert np.array_equal(bits(pose_a), bits(pose_b)) and np.array_equal(cnt_a, cnt_b)
    assert (cnt_a > np.array([m["n"] for m in duplicated["maps"]])).all()      # (the step appended rows)
    for b, (x, y) in enumerate(zip(bufs_a, bufs_b)):
        for k in range(4):
            assert np.array_equal(bits(x[k]), bits(y[k])), (b, k)


# ------------------------------------------------------------------------ 4: refusals
def _null(field, which):
    def spoil(seqs, t):
        for b in which:
            setattr(seqs[b], field, None)
    return spoil


def _give(field, tensor, which):
    def spoil(seqs, t):
        for b in which:
            setattr(seqs[b], field, t[tensor][b].data_ptr())
    return spoil


@pytest.mark.parametrize("outputs,spoil", [
    (True, _null("vertex", (0, 1, 2))),       # vertex NULL with alpha given
    (True, _null("alpha", (0, 1, 2))),        # the reverse
    (True, _null("vertex", (1,))),            # one sequence half-given
    (False, _give("vertex", "vertex", (0, 1, 2))),
    (True, lambda seqs, t: [setattr(seqs[2], k, None) for k in ("vertex", "alpha")]),   # a mixed choice across sequences
    (False, lambda seqs, t: [setattr(seqs[0], k, t[k][0].data_ptr()) for k in ("vertex", "alpha")]),
    (True, _null("best_pix", (1,))),          # best_pix: the same choice for every sequence too
], ids=["vertex-null", "alpha-null", "one-vertex-null", "vertex-without-alpha", "mixed-last", "mixed-first", "mixed-best"])
def test_half_given_outputs_are_refused(ops, duplicated, outputs, spoil):
    """the library's argument error, and nothing launched: the maps, the counts and the poses are untouched"""
    status, pose, cnt, bufs = _step_call(ops, duplicated, outputs, spoil)
    assert status == 1, status          # GS_ERR_INVALID
    from gradslam_amd import _C
    assert b"gs_pointfusion_step_batch_f32" in _C.lib().gs_last_error()
    assert not pose.any() and not cnt.any()
    for b, m in enumerate(duplicated["maps"]):
        for k in range(4):
            assert np.array_equal(bits(bufs[b][k]), bits(host(m["bufs"][k]))), (b, k)
