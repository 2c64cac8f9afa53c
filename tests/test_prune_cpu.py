"""CPU-only tests of the map prune: the NumPy restatement (tests/prune_ref.py) against hand-written cases, the host-side
argument validation of gs_prune_map_dc_f32 (it returns before any HIP call), CPU `Pointclouds.prune_ / prune /
mark_epoch` against the restatement, and the `PointFusion(prune_*=...)` arguments.

The operation moves bits, so every comparison is for equal bits."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from gradslam_amd.slam.pointfusion import PointFusion
from gradslam_amd.structures.pointclouds import Pointclouds
from tests import prune_ref as pr

NAN = float("nan")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ the restatement
def test_ref_boundary_equality_and_nan():
    cc = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), NAN, 0.75, -0.0, np.inf], np.float32)
    s = pr.survivors(6, cc, 0.5)
    assert s.tolist() == [True, False, False, True, False, True]       # equal stays, one ulp below goes, NaN goes
    # the comparison is float32: a threshold that rounds to 0.5 keeps 0.5
    assert pr.survivors(1, cc, 0.5 + 1e-12).tolist() == [True]
    # NaN rows that are young or without the confidence rule stay
    assert pr.survivors(6, cc, 0.5, marks=[2], young_mark=0).tolist() == [True, False, True, True, True, True]
    assert pr.survivors(6, cc, None).all()


def test_ref_keep_and_confidence_combine():
    cc = np.array([1, 0, 1, 0, 1], np.float32)
    keep = np.array([1, 1, 0, 0, 2], np.uint8)
    assert pr.survivors(5, cc, 0.5, keep).tolist() == [True, False, False, False, True]
    # young rows are still subject to keep
    assert pr.survivors(5, cc, 0.5, keep, marks=[0], young_mark=0).tolist() == [True, True, False, False, True]


def test_ref_rows_and_marks():
    P = np.arange(21, dtype=np.float32).reshape(7, 3)
    F = np.array([[0.1], [0.9], [0.2], [0.9], [0.9], [0.0], [0.0]], np.float32)
    # n = 6 of 7 rows: the last row lies beyond the count and never survives
    marks = [0, 2, 3, 6, 9]
    out = pr.prune(P, None, None, F, 6, 0.5, None, marks, 3)
    assert out[4] == 3 and out[5] == 3
    assert np.array_equal(out[0], P[[1, 3, 4]]) and out[1] is None and out[2] is None
    assert np.array_equal(bits(out[3]), bits(F[[1, 3, 4]]))
    assert out[6] == [0, 1, 1, 3, 3]           # marks at 0, inside, at n and beyond n
    # young_from = marks[1] = 2: rows 2.. are protected
    out = pr.prune(P, None, None, F, 6, 0.5, None, marks, 1)
    assert out[4] == 5 and out[6] == [0, 1, 2, 5, 5]


def test_ref_empty_map():
    P = np.zeros((0, 3), np.float32)
    F = np.zeros((0, 1), np.float32)
    out = pr.prune(P, P, P, F, 0, 0.5, None, [0, 4], 0)
    assert out[4] == 0 and out[5] == 0 and out[6] == [0, 0] and out[0].shape == (0, 3)
    out = pr.prune(np.ones((3, 3), np.float32), None, None, None, 0, None, np.ones(3, np.uint8))
    assert out[4] == 0 and out[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------ the C entry point
def _seq(**kw):
    """a descriptor that passes every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and
    every case below is rejected before one)"""
    d = dict(points=0x1000, normals=0x2000, colors=0x3000, features=0x4000, F=1, n_bound=100, n_dev=0,
             points_out=0x5000, normals_out=0x6000, colors_out=0x7000, features_out=0x8000, capacity_out=100,
             keep=0, marks=0x9000, n_marks=2, young_mark=1, n_out=0xa000, removed_out=0, scratch=0xb000)
    d.update(kw)
    return d


INVALID = {
    "null_points": (dict(points=0), "NULL"),
    "null_points_out": (dict(points_out=0), "NULL"),
    "null_normals_out": (dict(normals_out=0), "NULL"),
    "null_features_out": (dict(features_out=0), "NULL"),
    "null_n_out": (dict(n_out=0), "NULL"),
    "null_scratch": (dict(scratch=0), "NULL"),
    "null_marks": (dict(marks=0), "NULL"),
    "alias_points": (dict(points_out=0x1000), "alias"),
    "alias_normals": (dict(normals_out=0x2000), "alias"),
    "alias_colors": (dict(colors_out=0x3000), "alias"),
    "alias_features": (dict(features_out=0x4000), "alias"),
    "too_many_marks": (dict(n_marks=65), "n_marks"),
    "negative_marks": (dict(n_marks=-1, young_mark=-1), "n_marks"),
    "young_mark_high": (dict(young_mark=2), "young_mark"),
    "young_mark_low": (dict(young_mark=-2), "young_mark"),
    "negative_bound": (dict(n_bound=-1), "n_bound"),
    "capacity": (dict(capacity_out=99), "capacity"),
    "confidence_F3": (dict(F=3), "F == 1"),
    "confidence_no_features": (dict(features=0, features_out=0, F=0), "F == 1"),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_entry_point_rejects_before_any_hip_call(case):
    lib = _C.lib()
    change, word = INVALID[case]
    seqs = (_C.PruneSeq * 1)()
    for k, v in _seq(**change).items():
        setattr(seqs[0], k, v)
    assert lib.gs_prune_map_dc_f32(seqs, 1, 0.5, 1, None) == 1       # GS_ERR_INVALID
    assert word in lib.gs_last_error().decode(), lib.gs_last_error()


def test_entry_point_rejects_bad_batch_and_second_sequence():
    lib = _C.lib()
    seqs = (_C.PruneSeq * 2)()
    for q in seqs:
        for k, v in _seq().items():
            setattr(q, k, v)
    assert lib.gs_prune_map_dc_f32(None, 1, 0.5, 1, None) == 1
    assert lib.gs_prune_map_dc_f32(seqs, 0, 0.5, 1, None) == 1
    seqs[1].young_mark = 7        # every sequence is checked, not only the first
    assert lib.gs_prune_map_dc_f32(seqs, 2, 0.5, 1, None) == 1
    assert "young_mark" in lib.gs_last_error().decode()
    seqs[1].young_mark = 0
    assert lib.gs_prune_map_dc_f32(seqs, 2, float("nan"), 1, None) == 1
    assert "NaN" in lib.gs_last_error().decode()


def test_scratch_bytes_positive_and_monotone():
    lib = _C.lib()
    sizes = [lib.gs_prune_scratch_bytes(n) for n in (0, 1, 1023, 1024, 1025, 70001, 1 << 20, (1 << 20) + 5, 1 << 24)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.gs_prune_scratch_bytes(-5) == sizes[0]


def test_prune_kernels_use_no_scratch_and_spill_nothing():
    """All four passes are memory-bound streams over the map: a spill would add private-segment traffic to every row, and
    8 waves per SIMD (<= 64 VGPRs) keep enough loads and stores in flight."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_prune.hip", "gs_prune_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "gs_prune_" in ln and not ln.startswith("#")}
    assert set(rows) == {"gs_prune_count_kernel", "gs_prune_scan_kernel", "gs_prune_scatter_kernel",
                         "gs_prune_marks_kernel"}, r.stdout
    for name, (vgpr, sgpr, scratch, occ, sspill, vspill, lds) in rows.items():
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
        assert int(vgpr) <= 64 and int(occ) >= 8, (name, vgpr, occ)


def test_ops_have_no_cpu_fallback():
    from gradslam_amd import ops
    P = torch.zeros(4, 3)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.prune_map(P, None, None, torch.zeros(4, 1), min_confidence=0.5)
    with pytest.raises(_C.HipExtensionError, match="no CPU fallback"):
        ops.prune_map_batch([(P, None, None, None, 4, None)], keep=[torch.ones(4, dtype=torch.bool)])


# ------------------------------------------------------------------------------------------ CPU Pointclouds
NS = (50, 0, 33)


def ragged(seed=0, ns=NS, F=1):
    g = torch.Generator().manual_seed(seed)
    mk = lambda c: [torch.randn(n, c, generator=g) for n in ns]   # noqa: E731
    feats = [torch.rand(n, F, generator=g) for n in ns]
    return mk(3), mk(3), mk(3), feats


def as_ref(lists, b):
    return [None if a is None else a[b].numpy().copy() for a in lists]


def same_map(pc, b, want):
    """want: prune_ref.prune output"""
    got = (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)
    for g, w in zip(got, want[:4]):
        assert (g is None) == (w is None)
        if w is not None:
            a = g[b].detach().numpy()
            assert a.shape == w.shape and np.array_equal(bits(a), bits(w))
    assert pc._n[b] == want[4]
    assert int(pc.last_pruned[b]) == want[5]
    assert ([] if pc._marks is None else pc._marks[b, :pc._n_marks].tolist()) == want[6]


def test_pointclouds_prune_ragged_batch():
    lists = ragged()
    pc = Pointclouds(*lists)
    pc.mark_epoch()
    gen = pc._generation
    assert pc.prune_(0.5) is pc
    assert pc._generation > gen
    for b, n in enumerate(NS):
        same_map(pc, b, pr.prune(*as_ref(lists, b), n, 0.5, None, [n], -1))
    assert pc._n[1] == 0 and 0 < pc._n[0] < NS[0]


def test_pointclouds_prune_out_of_place_and_tensor_keep():
    lists = ragged(1, (40, 40))
    pc = Pointclouds(*lists)
    keep = torch.rand(2, 40, generator=torch.Generator().manual_seed(3)) < 0.7
    out = pc.prune(0.3, keep=keep)
    assert out is not pc and pc._n == [40, 40] and pc.last_pruned is None
    for b in range(2):
        same_map(out, b, pr.prune(*as_ref(lists, b), 40, 0.3, keep[b].numpy(), [], -1))
    # list form, uint8, only one sequence restricted
    out2 = pc.prune(keep=[keep[0].to(torch.uint8), torch.ones(40, dtype=torch.uint8)])
    same_map(out2, 0, pr.prune(*as_ref(lists, 0), 40, None, keep[0].numpy(), [], -1))
    assert out2._n[1] == 40


def test_marks_survive_two_prunes_and_min_age():
    lists = ragged(2)
    pc = Pointclouds(*lists)
    # epochs: pretend the rows came in three steps
    cuts = [[10, 0, 5], [30, 0, 20], list(NS)]
    pc._marks = torch.zeros((3, Pointclouds.MAX_MARKS), dtype=torch.int64)
    for k, c in enumerate(cuts):
        pc._marks[:, k] = torch.tensor(c)
    pc._n_marks = 3
    ref = [as_ref(lists, b) + [NS[b]] for b in range(3)]
    marks = [[c[b] for c in cuts] for b in range(3)]
    for conf, age in ((0.4, 2), (0.7, 3)):
        pc.prune_(conf, min_age=age)
        for b in range(3):
            w = pr.prune(*ref[b], conf, None, marks[b], 3 - age)
            same_map(pc, b, w)
            ref[b], marks[b] = list(w[:5]), w[6]
    assert sum(pc._n) < sum(NS)
    # more epochs asked for than recorded: every row is young, nothing goes
    n = list(pc._n)
    pc.prune_(0.99, min_age=4)
    assert pc._n == n and pc.last_pruned.tolist() == [0, 0, 0]
    # min_age = 0 protects nothing
    pc.prune_(0.99, min_age=0)
    for b in range(3):
        same_map(pc, b, pr.prune(*ref[b], 0.99, None, marks[b], -1))


def test_mark_ring_and_copies_carry_marks():
    lists = ragged(4)
    pc = Pointclouds(*lists)
    for _ in range(Pointclouds.MAX_MARKS + 3):
        pc.mark_epoch()
    assert pc._n_marks == Pointclouds.MAX_MARKS
    assert pc._marks[:, -1].tolist() == list(NS)
    pc._marks[:, :5] = 0
    pc._marks[0, 5] = 7
    for other in (pc.clone(), pc.detach(), pc.to("cpu", copy=True)):
        assert other._n_marks == pc._n_marks and torch.equal(other._marks, pc._marks)
        assert other._marks.data_ptr() != pc._marks.data_ptr()
    sub = pc[[2, 0]]
    assert torch.equal(sub._marks, pc._marks[[2, 0]]) and sub._n_marks == pc._n_marks


def test_prune_nan_and_boundary_confidence():
    P = torch.arange(12, dtype=torch.float32).reshape(1, 4, 3)
    F = torch.tensor([[[0.25], [NAN], [0.2499999], [0.25]]])
    pc = Pointclouds(P, P.clone(), P.clone(), F)
    pc.prune_(0.25)
    assert pc._n == [2] and torch.equal(pc.points_list[0], P[0, [0, 3]])


def test_prune_argument_errors():
    lists = ragged(5)
    with pytest.raises(ValueError, match="empty"):
        Pointclouds().prune_(0.5)
    with pytest.raises(ValueError, match="prune needs a surfel map: points, normals, colors and one feature channel"):
        Pointclouds(lists[0], lists[1]).prune_(0.5)
    with pytest.raises(ValueError, match="one feature channel"):
        Pointclouds(*ragged(5, F=3)).prune_(0.5)
    pc = Pointclouds(*lists)
    with pytest.raises(TypeError):
        pc.prune_("0.5")
    with pytest.raises(ValueError):
        pc.prune_(0.5, min_age=-1)
    with pytest.raises(ValueError):
        pc.prune_(keep=[torch.ones(50, dtype=torch.bool)])
    with pytest.raises(TypeError):
        pc.prune_(keep=[torch.ones(n) for n in NS])
    # F = 3 with keep only is fine
    pc3 = Pointclouds(*ragged(5, F=3))
    pc3.prune_(keep=[torch.zeros(n, dtype=torch.bool) for n in NS])
    assert pc3._n == [0, 0, 0]


def test_prune_keeps_rows_on_the_autograd_tape():
    lists = ragged(6, (20,))
    P = lists[0][0].clone().requires_grad_(True)
    pc = Pointclouds([P], lists[1], lists[2], lists[3])
    out = pc.prune(0.5)
    s = pr.survivors(20, lists[3][0].numpy()[:, 0], 0.5)
    out.points_list[0].sum().backward()
    assert np.array_equal(P.grad.numpy(), np.repeat(s[:, None], 3, 1).astype(np.float32))


# ------------------------------------------------------------------------------------------ PointFusion arguments
def test_pointfusion_prune_arguments():
    slam = PointFusion()
    assert slam.prune_min_confidence is None and slam.prune_min_age == 20 and slam.prune_every == 10
    slam = PointFusion(prune_min_confidence=0.01, prune_min_age=3, prune_every=2)
    assert (slam.prune_min_confidence, slam.prune_min_age, slam.prune_every) == (0.01, 3, 2)
    with pytest.raises(TypeError):
        PointFusion(prune_min_confidence="0.1")
    with pytest.raises(TypeError):
        PointFusion(prune_min_confidence=0.1, prune_min_age=2.0)
    with pytest.raises(TypeError):
        PointFusion(prune_min_confidence=0.1, prune_every=None)
    with pytest.raises(ValueError):
        PointFusion(prune_min_confidence=0.1, prune_every=0)
    with pytest.raises(ValueError):
        PointFusion(prune_min_confidence=0.1, prune_min_age=-1)
    with pytest.warns(UserWarning, match="non-negative"):
        PointFusion(prune_min_confidence=-0.1)
    with pytest.warns(UserWarning, match="64"):
        PointFusion(prune_min_confidence=0.1, prune_min_age=65)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        PointFusion(prune_min_confidence=0.1, prune_min_age=64)


class _CountingMap(Pointclouds):
    calls = None

    def mark_epoch(self):
        self.calls.append("mark")
        return super().mark_epoch()

    def prune_(self, *a, **kw):
        self.calls.append("prune")
        return super().prune_(*a, **kw)


class _NoKernels(PointFusion):
    """the schedule around a step without the kernels of the step (there is no GPU here): the step itself appends two
    rows of confidence 0 and 1"""

    def _localize(self, pointclouds, live_frame, prev_frame):
        return torch.eye(4).view(1, 1, 4, 4)

    def _map(self, pointclouds, live_frame, inplace=False):
        new = type(pointclouds)(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2, 3),
                                torch.tensor([[[0.0], [1.0]]]))
        return pointclouds.append_points(new)


def _fake_frame():
    from gradslam_amd.structures.rgbdimages import RGBDImages
    return RGBDImages(torch.zeros(1, 1, 2, 2, 3), torch.ones(1, 1, 2, 2, 1), torch.eye(4).view(1, 1, 4, 4),
                      torch.eye(4).view(1, 1, 4, 4))


def test_default_step_never_marks_or_prunes(monkeypatch):
    pc = _CountingMap()
    pc.calls = []
    slam = _NoKernels(odom="gt")
    for _ in range(12):
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=True)
    assert pc.calls == [] and pc._n == [24] and pc._prune_steps == 0 and pc._marks is None


def test_pruning_step_schedule():
    pc = _CountingMap()
    pc.calls = []
    slam = _NoKernels(odom="gt", prune_min_confidence=0.5, prune_min_age=1, prune_every=3)
    counts = []
    for _ in range(7):
        pc, _ = slam.step(pc, _fake_frame(), None, inplace=True)
        counts.append(pc._n[0])
    assert pc.calls == ["mark", "mark", "prune", "mark", "mark", "mark", "prune", "mark", "mark"]
    # step 3: the rows of steps 1, 2 are old (one of each pair goes), those of step 3 are protected; step 6 removes the
    # low row of steps 3, 4, 5
    assert counts == [2, 4, 4, 6, 8, 7, 9]
    assert pc._prune_steps == 7 and pc._n_marks == 7
