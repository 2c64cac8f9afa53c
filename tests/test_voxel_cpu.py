"""CPU-only tests of the voxel thinning: the NumPy restatement (tests/voxel_ref.py) against rows worked out by hand and
its properties on a seeded cloud, the torch path of Pointclouds.voxel_downsample_ against restatement + restated prune,
the effect on the oracle frame loop with the restated thinning between the frames, the host-side argument validation
of gs_voxel_keep_dc_f32 (it returns before any HIP call), and the arguments of ops.voxel_keep*, Pointclouds.voxel_* and
PointFusion(voxel_*=...).

The rule's outputs are integers and the removal moves bits, so every comparison of them is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from gradslam_amd.slam.pointfusion import PointFusion
from gradslam_amd.structures.pointclouds import Pointclouds, _voxel_keep_torch
from gradslam_amd.structures.rgbdimages import RGBDImages
from oracle import slam as oslam
from tests import prune_ref as pr
from tests import render_ref as rr
from tests import voxel_cases as vc
from tests import voxel_ref as vr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN, INF = vc.NAN, vc.INF
T = torch.from_numpy


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ the rule by hand
def test_ref_voxel_of_hand_made_rows():
    key, ok = vr.keys(vc.POINTS, vc.VS)
    assert key.dtype == np.uint64 and ok.tolist() == vc.GRIDDABLE.tolist()
    off = 1 << 20
    k = lambda x, y, z: ((x + off) << 42) | ((y + off) << 21) | (z + off)   # noqa: E731
    assert int(key[0]) == int(key[1]) == k(3, 0, 0) and int(key[2]) == k(2, 0, 0)
    assert int(key[3]) == int(key[4]) == k(-1, 0, 0), "-0.03 lands in voxel -1, not 0"
    assert int(key[5]) == int(key[6]) == k(0, 0, 0), "-0.0 is voxel 0"
    assert int(key[8]) == k(off - 1, 0, 0) and int(key[10]) == k(-off, 0, 0), "the limits of the grid"
    assert int(key[10]) == (off << 21) | off and int(key[8]) < 1 << 63, "63 bits: all-ones is never a key"
    assert int(key[25]) == k(80, 0, 0) and int(key[26]) == k(80, 1, 0) and int(key[27]) == k(80, 0, 1)
    assert f32(vc.BELOW) < f32(65536.0) and f32(vc.BEYOND) < f32(-65536.0)


def test_ref_scores_order_like_the_confidences():
    c = np.array([NAN, -5.0, -0.0, 0.0, 1e-45, 0.25, 3.0, 1e30, INF, -INF], f32)
    s = vr.scores(c, c.size)
    assert s.dtype == np.uint32 and s[:4].tolist() == [0, 0, 0, 0] and s[9] == 0 and s[4] == 1
    assert (np.diff(s[3:9].astype(np.int64)) > 0).all() and s[8] == 0x7F800000
    assert vr.scores(None, 4).tolist() == [0] * 4


def test_ref_winners_of_hand_made_rows():
    n = len(vc.ROWS)
    keep, winner = vr.voxel_keep(vc.POINTS, vc.CONF, n, vc.VS)
    assert keep.dtype == np.uint8 and winner.dtype == np.int64
    assert winner.tolist() == vc.WINNER.tolist()
    assert keep.tolist() == (vc.WINNER == np.arange(n)).astype(int).tolist()
    assert keep[7] == 1 and keep[9] == 1, "two identical rows out of range are both kept"
    # (rows, 1) confidences, as a map holds them
    keep2, winner2 = vr.voxel_keep(vc.POINTS, vc.CONF[:, None], n, vc.VS)
    assert np.array_equal(keep2, keep) and np.array_equal(winner2, winner)
    # no confidence at all: the first row of a voxel
    keep, winner = vr.voxel_keep(vc.POINTS, None, n, vc.VS)
    assert winner.tolist() == vc.WINNER_PLAIN.tolist()
    assert keep.tolist() == (vc.WINNER_PLAIN == np.arange(n)).astype(int).tolist()


def test_ref_rows_beyond_the_count_get_zero_and_never_compete():
    keep, winner = vr.voxel_keep(vc.POINTS, vc.CONF, 19, vc.VS)
    assert keep[19:].tolist() == [0] * (len(vc.ROWS) - 19) and winner[19:].tolist() == [-1] * (len(vc.ROWS) - 19)
    assert winner[18] == 18 and keep[18] == 1, "the +inf confidence of row 19 lies beyond the count"
    assert winner[:18].tolist() == vc.WINNER[:18].tolist()
    keep, winner = vr.voxel_keep(vc.POINTS, vc.CONF, 0, vc.VS)
    assert not keep.any() and (winner == -1).all()


def test_torch_rule_equals_the_restatement():
    for P, C in ((vc.POINTS, vc.CONF), vc.cloud()):
        for conf in (C, None):
            for vs in (vc.VS, 0.05, 2.0 ** -6):
                vs32 = float(f32(vs))
                want = vr.voxel_keep(P, conf, P.shape[0], vs32)
                got = _voxel_keep_torch(T(P), None if conf is None else T(conf), vs32)
                assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int64
                assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), vs
    k, w = _voxel_keep_torch(torch.zeros(0, 3), None, 0.5)
    assert k.shape == (0,) and w.shape == (0,)


# ------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("vs", [0.0625, 0.05, 0.3])
def test_properties_on_a_seeded_cloud(vs):
    P, C = vc.cloud(5000)
    n = P.shape[0]
    keep, winner = vr.voxel_keep(P, C, n, vs)
    key, ok = vr.keys(P, vs)
    assert 0 < (~ok).sum() < n // 50
    survivors = np.nonzero(keep)[0]
    gs = survivors[ok[survivors]]
    assert np.unique(key[gs]).size == gs.size, "at most one griddable survivor per voxel"
    assert set(key[gs].tolist()) == set(key[ok].tolist()), "every voxel that had a row has one"
    assert keep[~ok].all() and (winner[~ok] == np.nonzero(~ok)[0]).all(), "rows off the grid are kept"
    assert np.array_equal(winner[winner], winner), "winner[winner] == winner"
    assert np.array_equal(key[winner[ok]], key[ok]), "a winner lives in the voxel it wins"
    assert 0 < survivors.size < n
    # the winner has the largest score of its voxel, and is the lowest row among those
    sc = vr.scores(C, n)
    for v in np.unique(key[ok])[:200]:
        rows = np.nonzero(ok & (key == v))[0]
        top = rows[sc[rows] == sc[rows].max()][0]
        assert (winner[rows] == top).all()
    # idempotent: a second pass over the compacted cloud removes nothing
    s = keep != 0
    keep2, winner2 = vr.voxel_keep(P[s], C[s], int(s.sum()), vs)
    assert keep2.all() and np.array_equal(winner2, np.arange(int(s.sum())))


# ------------------------------------------------------------------------------------------ Pointclouds on the CPU
def _cpu_maps(counts=(5000, 28), marks=True):
    arrs = []
    for b, n in enumerate(counts):
        rng = np.random.default_rng(90 + b)
        P, C = (vc.POINTS, vc.CONF) if n == len(vc.ROWS) else vc.cloud(n, seed=11 + b)
        raw = lambda c: rng.integers(0, 1 << 32, size=(n, c), dtype=np.uint64).astype(np.uint32).view(f32)  # noqa: E731
        arrs.append((P.copy(), raw(3), raw(3), C.reshape(-1, 1).copy()))
    pc = Pointclouds(*[[T(a[i].copy()) for a in arrs] for i in range(4)])
    if marks:
        pc.mark_epoch()
        pc._marks[:, 0] //= 3
        pc.mark_epoch()
        pc._marks[:, 1] //= 2
    return pc, arrs


def test_pointclouds_voxel_downsample_on_cpu_equals_restatement_and_restated_prune():
    counts = (5000, len(vc.ROWS))
    pc, arrs = _cpu_maps(counts)
    winners = pc.voxel_winners(vc.VS)
    gen = pc._generation
    assert pc.voxel_downsample_(vc.VS) is pc and pc._generation > gen
    for b, n in enumerate(counts):
        keep, winner = vr.voxel_keep(arrs[b][0], arrs[b][3], n, vc.VS)
        assert winners[b].dtype == torch.int64 and np.array_equal(winners[b].numpy(), winner), b
        want = pr.prune(*arrs[b], n, None, keep, [n // 3, n // 2], -1)
        assert 0 < want[5] < n
        assert pc._n[b] == want[4] and int(pc.last_pruned[b]) == want[5]
        assert pc._marks[b, :2].tolist() == want[6], "the epoch marks are rewritten"
        for k, a in zip(("points", "normals", "colors", "features"), want[:4]):
            got = getattr(pc, k + "_list")[b].numpy()
            assert got.shape == a.shape and np.array_equal(bits(got), bits(a)), (b, k)
    assert pc.last_pruned.dtype == torch.int64
    # a second pass removes nothing
    before = [t.clone() for t in pc.points_list]
    pc.voxel_downsample_(vc.VS)
    assert pc.last_pruned.tolist() == [0, 0] and all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                     for a, b in zip(before, pc.points_list))


def test_out_of_place_form_leaves_the_source_alone_and_taped_rows_stay_on_the_tape():
    pc, arrs = _cpu_maps((300,), marks=False)
    out = pc.voxel_downsample(0.25)
    keep = vr.voxel_keep(arrs[0][0], arrs[0][3], 300, 0.25)[0] != 0
    assert out is not pc and pc._n == [300] and pc.last_pruned is None
    assert out._n == [int(keep.sum())] and 0 < keep.sum() < 300
    assert np.array_equal(bits(pc.points_list[0].numpy()), bits(arrs[0][0]))
    # on the tape: the kept rows stay on it
    ok = np.isfinite(arrs[0][0]).all(1)
    Pg = T(np.where(ok[:, None], arrs[0][0], 0).astype(f32)).requires_grad_(True)
    taped = Pointclouds([Pg], [T(arrs[0][1])], [T(arrs[0][2])], [T(arrs[0][3])])
    thin = taped.voxel_downsample(0.25)
    keep = vr.voxel_keep(Pg.detach().numpy(), arrs[0][3], 300, 0.25)[0] != 0
    assert thin.points_list[0].requires_grad and thin._n == [int(keep.sum())]
    thin.points_list[0].sum().backward()
    assert np.array_equal(Pg.grad.numpy(), np.repeat(keep[:, None], 3, 1).astype(f32))


def test_a_map_with_another_feature_layout_is_thinned_with_every_score_zero():
    P, C = vc.cloud(400, seed=3)
    feats = np.random.default_rng(0).random((400, 3)).astype(f32)
    pc = Pointclouds([T(P)], None, None, [T(feats)])
    pc.voxel_downsample_(0.25)
    keep = vr.voxel_keep(P, None, 400, 0.25)[0] != 0
    assert np.array_equal(bits(pc.features_list[0].numpy()), bits(feats[keep]))
    plain = Pointclouds([T(P)])
    assert np.array_equal(plain.voxel_winners(0.25)[0].numpy(), vr.voxel_keep(P, None, 400, 0.25)[1])


# ------------------------------------------------------------------------------------------ refusals
BAD_SIZES = [(0, ValueError), (0.0, ValueError), (-0.1, ValueError), (NAN, ValueError), (INF, ValueError),
             (1e-60, ValueError), (True, TypeError), ("0.1", TypeError), (None, TypeError)]


@pytest.mark.parametrize("method", ["voxel_downsample_", "voxel_downsample", "voxel_winners"])
def test_pointclouds_voxel_argument_errors(method):
    pc, _ = _cpu_maps((40,), marks=False)
    for val, exc in BAD_SIZES:
        with pytest.raises(exc, match="voxel_size"):
            getattr(pc, method)(val)
    with pytest.raises(ValueError, match="empty"):
        getattr(Pointclouds(), method)(0.1)
    assert pc._n == [40] and pc.last_pruned is None


def test_ops_have_no_cpu_fallback_and_name_the_argument():
    from gradslam_amd import ops
    P, C = T(vc.POINTS), T(vc.CONF)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.voxel_keep(P, vc.VS)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.voxel_keep(P, vc.VS, C)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.voxel_keep_batch([(P, None, None, C[:, None], None, None)], vc.VS)
    for val, exc in BAD_SIZES:
        with pytest.raises(exc, match="voxel_size"):
            ops.voxel_keep(P, val)
        with pytest.raises(exc, match="voxel_size"):
            ops.voxel_keep_batch([(P, None, None, None, None, None)], val)
        with pytest.raises(exc, match="voxel_size"):
            ops._voxel_args("somebody", val)
    assert ops._voxel_args("x", 0.1) == float(f32(0.1)) and ops._voxel_args("x", 1) == 1.0
    with pytest.raises(TypeError, match="points"):
        ops.voxel_keep(vc.POINTS, vc.VS)
    with pytest.raises(ValueError, match="confidence"):
        ops.voxel_keep(P, vc.VS, torch.zeros(len(vc.ROWS), 2))
    with pytest.raises(ValueError, match="maps"):
        ops.voxel_keep_batch([], vc.VS)
    with pytest.raises(ValueError, match="points"):
        ops.voxel_keep_batch([(torch.zeros(5, 4), None, None, None, None, None)], vc.VS)
    with pytest.raises(ValueError, match="features"):
        ops.voxel_keep_batch([(torch.zeros(5, 3), None, None, torch.zeros(4, 1), None, None)], vc.VS)
    with pytest.raises(ValueError, match="out"):
        ops.voxel_keep_batch([(P, None, None, None, None, None)], vc.VS, out=([None],))


def test_pointfusion_voxel_arguments():
    slam = PointFusion()
    assert slam.voxel_size is None and slam.voxel_every == 1
    slam = PointFusion(voxel_size=2 ** -6, voxel_every=3)
    assert (slam.voxel_size, slam.voxel_every) == (2 ** -6, 3)
    assert PointFusion(voxel_size=1).voxel_size == 1
    for kw in (dict(voxel_size="0.1"), dict(voxel_size=True), dict(voxel_size=0.1, voxel_every=1.0),
               dict(voxel_size=0.1, voxel_every=None), dict(voxel_every=False)):
        with pytest.raises(TypeError):
            PointFusion(**kw)
    for kw in (dict(voxel_size=0), dict(voxel_size=-0.1), dict(voxel_size=NAN), dict(voxel_size=INF),
               dict(voxel_size=0.1, voxel_every=0), dict(voxel_every=0), dict(voxel_every=-2)):
        with pytest.raises(ValueError):
            PointFusion(**kw)
    from gradslam_amd.slam.icpslam import ICPSLAM
    with pytest.raises(TypeError):
        ICPSLAM(voxel_size=0.05)       # like pruning and carving, thinning is a map-fusion feature


# ------------------------------------------------------------------------------------------ the step schedule
class _CountingMap(Pointclouds):
    calls = []       # of the class: an out-of-place step makes new containers

    def mark_epoch(self):
        self.calls.append("mark")
        return super().mark_epoch()

    def prune_(self, *a, **kw):
        self.calls.append("prune")
        return super().prune_(*a, **kw)

    def carve_(self, frames, **kw):
        self.calls.append("carve")
        return self

    def voxel_downsample_(self, voxel_size):
        self.calls.append(("voxel", voxel_size))
        return super().voxel_downsample_(voxel_size)      # (its removal is a prune_: recorded as one)


class _TwoRowsAStep(PointFusion):
    """the schedule around a step without the kernels of the step: a step appends the same two rows, one of confidence 0
    and one of confidence 1 + the step number"""
    steps = 0

    def _localize(self, pointclouds, live_frame, prev_frame):
        return torch.eye(4).view(1, 1, 4, 4) * 1.0

    def _map(self, pointclouds, live_frame, inplace=False):
        self.steps += 1
        x = torch.tensor([[[0.01, 0.01, 0.01], [0.51, 0.01, 0.01]]])
        new = type(pointclouds)(x, torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.tensor([[[0.0], [1.0 + self.steps]]]))
        if inplace:
            return pointclouds.append_points(new)
        out = type(pointclouds)()
        if pointclouds.has_points:
            out.append_points(pointclouds)
        return out.append_points(new)


def _fake_frame():
    return RGBDImages(torch.zeros(1, 1, 2, 2, 3), torch.ones(1, 1, 2, 2, 1), torch.eye(4).view(1, 1, 4, 4),
                      torch.eye(4).view(1, 1, 4, 4))


def test_default_step_never_thins():
    pc = _CountingMap()
    del _CountingMap.calls[:]
    slam = _TwoRowsAStep(odom="gt")
    for _ in range(4):
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=True)
    assert pc.calls == [] and pc._voxel_steps == 0 and pc._n == [8]


@pytest.mark.parametrize("inplace", [True, False])
def test_thinning_step_schedule_order_and_effect(inplace):
    pc = _CountingMap()
    del _CountingMap.calls[:]
    slam = _TwoRowsAStep(odom="gt", voxel_size=0.25, voxel_every=2, carve_margin=0.03, prune_min_confidence=0.5,
                         prune_min_age=1, prune_every=4)
    sizes = []
    for _ in range(4):
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=inplace)
        sizes.append(list(pc._n))
    # carve -> thin -> prune schedule, in every step that has them
    assert pc.calls == ["carve", "mark", "carve", ("voxel", 0.25), "prune", "mark", "carve", "mark", "carve",
                        ("voxel", 0.25), "prune", "prune", "mark"]
    assert pc._voxel_steps == 4 and pc.clone()._voxel_steps == 4
    # two voxels: a thinning step leaves one row in each.  The rows of the first all score 0, so the oldest stays; in the
    # second the newest is the most confident.  The thinning of step 4 rewrites the newest mark from 4 to 1 (one survivor
    # in front of it), so the prune that follows finds row 0 old and unconfident, and the winner of the second voxel young
    assert sizes == [[2], [2], [4], [1]]
    assert pc.features_list[0][:, 0].tolist() == [5.0]
    assert pc._marks[0, :pc._n_marks].tolist() == [0, 0, 0, 1]


# ------------------------------------------------------------------------------------------ the effect
# the oracle frame loop with ground-truth poses on make_sequence(20, 60, 80, seed=0), sigma 0.6, gates 0.05 m / 20 deg;
# with thinning, voxel_ref.thin_map(m, 2**-6) after every frame.  Rows after frames 0, 9 and 19, and the RMSE of the last
# model view against its frame (tests/render_ref.py), as the restatement produced them:
EFFECT = {"wave": ((4556, 10433, 14505), (4556, 7706, 9330), 0.005266663582285261, 0.00497125272243897),
          "facets": ((4556, 10476, 14593), (4556, 7668, 9225), 0.0031913721735271497, 0.0029699211393100586)}


def _loop(s, voxel_size=None):
    Kc = s["intrinsics"][0]
    rows = []

    def per_frame(i, m, pose):
        if voxel_size is not None:
            vr.thin_map(m, voxel_size)
        rows.append(len(m))

    m, poses = oslam.run_sequence(s["colors"], s["depths"], Kc, s["poses"], odom="gt", per_frame=per_frame)
    r = rr.render(m.points, m.normals, m.colors, m.ccounts, poses[-1], Kc, 60, 80)
    return m, rows, rr.residual_stats(r.depth, s["depths"][-1])


@pytest.mark.parametrize("scene", ["wave", "facets"])
def test_thinning_every_frame_removes_a_third_of_the_map_and_the_model_view_is_no_worse(scene):
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(20, 60, 80, seed=0, scene=scene)
    rows0, rows1, rmse0, rmse1 = EFFECT[scene]
    plain, rows, st0 = _loop(s)
    print(scene, "without thinning: rows", rows, "rmse", st0["rmse"], "coverage", st0["coverage"])
    assert (rows[0], rows[9], rows[19]) == rows0
    assert st0["rmse"] == pytest.approx(rmse0, rel=1e-9)
    thin, rows, st1 = _loop(s, 2.0 ** -6)
    print(scene, "thinned every frame: rows", rows, "rmse", st1["rmse"], "coverage", st1["coverage"])
    assert (rows[0], rows[9], rows[19]) == rows1
    assert st1["rmse"] == pytest.approx(rmse1, rel=1e-9)
    # thinning should not make the model view worse; which surfel wins a pixel may change: 5 % is a judgement
    assert st1["rmse"] <= 1.05 * st0["rmse"]
    assert rows1[2] < 0.7 * rows0[2], "about a third of the rows are gone"
    assert vr.thin_map(thin, 2.0 ** -6) == 0, "idempotent on a real map"


# ------------------------------------------------------------------------------------------ the C entry point
@pytest.mark.parametrize("case", sorted(vc.INVALID))
def test_entry_point_rejects_before_any_hip_call(case):
    vc.check_refusal(_C, case)


def test_entry_point_checks_every_sequence_and_sizes_the_table():
    vc.check_refusals_of_the_batch(_C)


def test_symbols_are_exported_and_the_abi_version_stays():
    for name in ("gs_voxel_keep_scratch_bytes", "gs_voxel_keep_dc_f32"):
        assert name in _C.EXPORTS and hasattr(_C.lib(), name)
    assert _C.ABI_VERSION == 3 and _C.lib().gs_abi_version() == 3          # additions only
    hdr = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    assert "gs_voxel_keep_dc_f32(" in hdr and "typedef struct gs_voxel_keep_seq" in hdr
    import ctypes as C
    assert C.sizeof(_C.VoxelKeepSeq) == 9 * 8
    # the rule stands verbatim in the kernel's header comment and in the restatement
    src = open(os.path.join(REPO, "gradslam_amd", "csrc", "gs_voxel.hip")).read()
    for phrase in ("Voxel of a row.", "Griddable rows.", "Key.", "Score of a row.", "Winner.", "Keep mask.",
                   "Winner output."):
        assert phrase in src and phrase in vr.__doc__, phrase


def test_voxel_kernels_use_no_scratch_no_lds_and_spill_nothing():
    """two latency-bound passes of scattered atomics and gathers: full occupancy (8 waves per SIMD) keeps them in flight"""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_voxel.hip", "gs_voxel_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_voxel_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_voxel_elect_kernel", "gs_voxel_resolve_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0 and int(lds) == 0, (name, scratch, lds)
        assert int(vgpr) <= 64 and int(occ) >= 8, (name, vgpr, occ)
