"""GPU tests of the voxel thinning (gs_voxel.hip -> gs_voxel_keep_dc_f32 -> ops.voxel_keep_batch ->
Pointclouds.voxel_downsample_ -> PointFusion(voxel_size=...)) against its NumPy restatement (tests/voxel_ref.py), the
CPU path of Pointclouds and, end to end, the oracle frame loop that applies the restatement between the frames.

The outputs of the pass are integers and the removal moves bits, so every comparison is for EQUALITY: no tolerance
anywhere.  Block = 256 rows, 8 sequences per launch, a table of max(2 n_bound, 1024) slots rounded up to a power of two:
the sizes sit on and around those."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from oracle import slam as oslam
from tests import prune_ref as pr
from tests import voxel_cases as vc
from tests import voxel_ref as vr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
f32 = np.float32
NROWS, VS = 1027, 0.125          # 1027 rows in a cube of 1 m: 512 voxels of 0.125 m, two rows each on average
PAD, SENT8, SENT64 = 13, 0xAB, -77   # elements beyond n_bound, and values the pass never writes


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


_FIX = {}


def fixture_data():
    """(points (1027, 3), confidence (1027,)); computed once and never changed"""
    if "d" not in _FIX:
        _FIX["d"] = vc.cloud(NROWS, seed=5)
    return _FIX["d"]


_REF = {}


def ref(n, n_bound=None, conf=True, vs=VS):
    """the restatement on the first n rows of the fixture (cached: the references are shared and left alone)"""
    key = (n, n_bound, conf, vs)
    if key not in _REF:
        P, C = fixture_data()
        nb = n if n_bound is None else n_bound
        _REF[key] = vr.voxel_keep(P[:nb], C[:nb] if conf else None, n, vs)
    return _REF[key]


def run(ops, P, C, n_dev=None, vs=VS, want=(True, True)):
    """ops.voxel_keep_batch of one map into sentinel-filled outputs with PAD elements beyond n_bound: every element up to
    the bound must have been written, none beyond it.  Returns (keep, winner, unplaced) on the host."""
    rows = P.shape[0]
    k = torch.full((rows + PAD,), SENT8, dtype=torch.uint8, device="cuda")
    w = torch.full((rows + PAD,), SENT64, dtype=torch.int64, device="cuda")
    out = ([k[:rows]] if want[0] else None, [w[:rows]] if want[1] else None)
    feats = None if C is None else dev(np.asarray(C, f32).reshape(-1, 1))
    r = ops.voxel_keep_batch([(dev(P), None, None, feats, None, n_dev)], vs, out=out)
    assert r.unplaced.dtype == torch.int32 and r.unplaced.shape == (1,) and r.unplaced.is_cuda
    assert (host(k[rows:]) == SENT8).all() and (host(w[rows:]) == SENT64).all(), "written beyond n_bound"
    assert (r.keep[0] is None) == (not want[0]) and (r.winner[0] is None) == (not want[1])
    if not want[0]:
        assert (host(k) == SENT8).all()
    if not want[1]:
        assert (host(w) == SENT64).all()
    return host(k[:rows]), host(w[:rows]), host(r.unplaced)


# ------------------------------------------------------------------------------------------ kernel == restatement
@pytest.mark.parametrize("n", [1, 255, 256, 257, NROWS])
def test_kernel_equals_restatement(ops, n):
    P, C = fixture_data()
    for conf in (True, False):
        keep, winner, unplaced = run(ops, P[:n], C[:n] if conf else None)
        want = ref(n, conf=conf)
        assert keep.dtype == np.uint8 and winner.dtype == np.int64
        assert np.array_equal(winner, want[1]), (conf, np.nonzero(winner != want[1])[0][:10])
        assert np.array_equal(keep, want[0]), conf
        assert unplaced.tolist() == [0]
        again = run(ops, P[:n], C[:n] if conf else None)
        assert np.array_equal(again[0], keep) and np.array_equal(again[1], winner), "a second run gives the same bits"
    if n == NROWS:
        assert 0 < ref(n)[0].sum() < n and not np.array_equal(ref(n)[1], ref(n, conf=False)[1])


def test_table_at_exactly_half_load(ops):
    """512 rows in 512 distinct voxels: the table of max(2 * 512, 1024) = 1024 slots is half full"""
    assert _C.lib().gs_voxel_keep_scratch_bytes(512) == 1024 * 16
    g = np.arange(8, dtype=f32)
    P = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) - f32(3.5)) * f32(VS)
    rng = np.random.default_rng(1)
    P = np.ascontiguousarray(P[rng.permutation(512)], f32)
    assert np.unique(vr.keys(P, VS)[0]).size == 512
    keep, winner, unplaced = run(ops, P, rng.random(512).astype(f32))
    assert keep.tolist() == [1] * 512 and winner.tolist() == list(range(512)) and unplaced.tolist() == [0]


def test_rows_beyond_the_device_count_get_zero_and_never_compete(ops):
    P, C = fixture_data()
    n = 700
    Q, D = P.copy(), C.copy()
    Q[n:], D[n:] = Q[:NROWS - n], np.inf        # beyond the count: rows of occupied voxels with the highest confidence
    n_dev = torch.tensor([n], dtype=torch.int64, device="cuda")
    keep, winner, unplaced = run(ops, Q, D, n_dev)
    want = ref(n, NROWS)
    assert np.array_equal(keep[:n], want[0][:n]) and np.array_equal(winner[:n], want[1][:n])
    assert (keep[n:] == 0).all() and (winner[n:] == -1).all() and unplaced.tolist() == [0]
    assert keep[:n].any() and (keep[:n] == 0).any()
    full = vr.voxel_keep(Q, D, NROWS, VS)
    assert full[0][n:].any() and not np.array_equal(full[1][:n], winner[:n]), "they would win if they were read"
    # NaN rows beyond the count are not read either; a device count above the bound is clamped to the bound
    Q[n:] = np.nan
    keep2, winner2, _ = run(ops, Q, D, n_dev)
    assert np.array_equal(keep2, keep) and np.array_equal(winner2, winner)
    big = torch.tensor([NROWS + 50], dtype=torch.int64, device="cuda")
    keep3, winner3, _ = run(ops, P, C, big)
    assert np.array_equal(keep3, ref(NROWS)[0]) and np.array_equal(winner3, ref(NROWS)[1])


@pytest.mark.parametrize("counts", [(257,), (NROWS, 0, 300), (5, 1024, 257, 0, NROWS, 1, 513, 64, 1000)])
def test_batch_equals_single_calls(ops, counts):
    """B = 1, B = 3 in one launch group and B = 9 in two: every sequence as in a call of its own, and as the restatement;
    ragged bounds, the odd sequences with a device count 9 rows below their bound"""
    P, C = fixture_data()
    maps, wants = [], []
    for b, n in enumerate(counts):
        extra = (b % 2) * 9
        Pb = np.roll(P, -37 * b, axis=0)[:n + extra]
        Cb = np.roll(C, -37 * b)[:n + extra].copy()
        Cb[n:] = np.inf
        n_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if b % 2 else None
        maps.append((dev(Pb), None, None, dev(Cb.reshape(-1, 1)), None, n_dev))
        wants.append(vr.voxel_keep(Pb, Cb, n, VS))
        one = ops.voxel_keep(maps[b][0], VS, maps[b][3], n_dev)
        assert np.array_equal(host(one.keep), wants[b][0]) and np.array_equal(host(one.winner), wants[b][1]), b
        assert host(one.unplaced).tolist() == [0]
    got = ops.voxel_keep_batch(maps, VS)
    assert len(got.keep) == len(got.winner) == len(counts) and got.unplaced.shape == (len(counts),)
    assert host(got.unplaced).tolist() == [0] * len(counts)
    for b, want in enumerate(wants):
        assert got.keep[b].dtype == torch.uint8 and got.winner[b].dtype == torch.int64
        assert np.array_equal(host(got.keep[b]), want[0]) and np.array_equal(host(got.winner[b]), want[1]), b


# ------------------------------------------------------------------------------------------ special cases
def test_hand_made_rows(ops):
    n = len(vc.ROWS)
    keep, winner, unplaced = run(ops, vc.POINTS, vc.CONF, vs=vc.VS)
    assert winner.tolist() == vc.WINNER.tolist(), [(i, vc.ROWS[i][4]) for i in np.nonzero(winner != vc.WINNER)[0]]
    assert keep.tolist() == (vc.WINNER == np.arange(n)).astype(int).tolist() and unplaced.tolist() == [0]
    keep, winner, _ = run(ops, vc.POINTS, None, vs=vc.VS)
    assert winner.tolist() == vc.WINNER_PLAIN.tolist()
    assert keep.tolist() == (vc.WINNER_PLAIN == np.arange(n)).astype(int).tolist()
    # a count on the device that cuts the +inf confidence of row 19 off
    keep, winner, _ = run(ops, vc.POINTS, vc.CONF, torch.tensor([19], dtype=torch.int64, device="cuda"), vs=vc.VS)
    want = vr.voxel_keep(vc.POINTS, vc.CONF, 19, vc.VS)
    assert np.array_equal(keep, want[0]) and np.array_equal(winner, want[1]) and winner[18] == 18
    # a features tensor of another layout does not compete: every score is 0
    r = ops.voxel_keep_batch([(dev(vc.POINTS), None, None, dev(np.tile(vc.CONF[:, None], (1, 2))), None, None)], vc.VS)
    assert host(r.winner[0]).tolist() == vc.WINNER_PLAIN.tolist()


def test_all_rows_in_one_voxel(ops):
    """pure contention on one slot: 1027 rows, four blocks, one atomicMax target"""
    rng = np.random.default_rng(3)
    P = rng.uniform(0.26, 0.37, (NROWS, 3)).astype(f32)          # inside voxel (2, 2, 2) of 0.125 m
    assert np.unique(vr.keys(P, VS)[0]).size == 1
    for C in (rng.integers(0, 4, NROWS).astype(f32), np.full(NROWS, 2.5, f32), None):
        keep, winner, unplaced = run(ops, P, C)
        want = vr.voxel_keep(P, C, NROWS, VS)
        assert np.array_equal(keep, want[0]) and np.array_equal(winner, want[1])
        assert keep.sum() == 1 and (winner == winner[0]).all() and unplaced.tolist() == [0]
    assert winner[0] == 0, "without confidences the first row"


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_keys_that_differ_in_one_axis_only(ops, axis):
    """300 voxels in a row along one axis, two rows in each: a field of the key that was dropped or shifted wrong would
    merge them"""
    rng = np.random.default_rng(axis)
    i = np.repeat(np.arange(-150, 150), 2)[rng.permutation(600)]
    P = np.full((600, 3), 0.3, f32)
    P[:, axis] = (i.astype(f32) + f32(0.5)) * f32(VS)
    C = rng.random(600).astype(f32)
    keep, winner, unplaced = run(ops, P, C)
    want = vr.voxel_keep(P, C, 600, VS)
    assert np.array_equal(keep, want[0]) and np.array_equal(winner, want[1])
    assert keep.sum() == 300 and unplaced.tolist() == [0]


def test_either_output_may_be_left_out(ops):
    P, C = fixture_data()
    want = ref(NROWS)
    keep, _, _ = run(ops, P, C, want=(True, False))
    assert np.array_equal(keep, want[0])
    _, winner, _ = run(ops, P, C, want=(False, True))
    assert np.array_equal(winner, want[1])
    Pd = dev(P)
    with pytest.raises(ValueError, match="out"):
        ops.voxel_keep_batch([(Pd, None, None, None, None, None)], VS, out=([None], [None]))
    with pytest.raises(ValueError, match="out"):
        ops.voxel_keep_batch([(Pd, None, None, None, None, None)], VS,
                             out=([torch.zeros(5, dtype=torch.uint8, device="cuda")], None))
    # nothing is on the tape, and a requires-grad input says so
    Pg = Pd.clone().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="detached"):
        r = ops.voxel_keep(Pg, VS, dev(C))
    assert not r.winner.requires_grad and np.array_equal(host(r.winner), want[1])
    # an empty map: nothing to write
    r = ops.voxel_keep(torch.zeros(0, 3, device="cuda"), VS)
    assert r.keep.shape == (0,) and r.winner.shape == (0,) and host(r.unplaced).tolist() == [0]


# ------------------------------------------------------------------------------------------ Pointclouds
def device_map(gs, counts, extra=300):
    """a Pointclouds whose counts live on the device (one group), on buffers with `extra` rows of room that hold rows of
    occupied voxels with an infinite confidence; rows of the fixture, other attributes of random bits"""
    P, C = fixture_data()
    B = len(counts)
    pc = gs.Pointclouds(device="cuda")
    pc._init_empty_batch(B, 1)
    arrs = []
    for b, n in enumerate(counts):
        rng = np.random.default_rng(50 + b)
        Pb = np.concatenate([np.roll(P, -11 * b, axis=0)[:n], np.resize(P[:max(n, 1)], (extra, 3))]).astype(f32)
        Cb = np.concatenate([np.roll(C, -11 * b)[:n], np.full(extra, np.inf, f32)]).astype(f32)
        raw = lambda c: rng.integers(0, 1 << 32, size=(n + extra, c), dtype=np.uint64).astype(np.uint32).view(f32)  # noqa: E731
        arrs.append((Pb, raw(3), raw(3), Cb.reshape(-1, 1)))
        for k, a in zip(("points", "normals", "colors", "features"), arrs[-1]):
            pc._buf[k][b] = dev(a)
    cnt = torch.tensor(counts, dtype=torch.int64, device="cuda")
    pc._n_host[:] = list(counts)
    pc._set_counts_dev(cnt, 0)
    pc._set_counts_dev(cnt, extra)
    torch.cuda.synchronize()
    pc._dcount[0].group.poll()
    assert pc._dcount[0].group.bounds == [n + extra for n in counts] and not pc._dcount[0].group._pending
    return pc, arrs


def cpu_map(gs, arrs, counts):
    return gs.Pointclouds(*[[T(a[i][:n].copy()) for a, n in zip(arrs, counts)] for i in range(4)])


def test_pointclouds_voxel_downsample_on_the_device_equals_the_cpu_path(gs):
    counts = (NROWS, 300)
    pc, arrs = device_map(gs, counts)
    cpu = cpu_map(gs, arrs, counts)
    for m in (pc, cpu):
        m.mark_epoch()
        m._marks[:, 0] //= 2                      # an older epoch, somewhere inside the maps
    winners = pc.voxel_winners(VS)
    assert len(pc._dcount) == 2, "reading the winners resolved a device-side count"
    for b, n in enumerate(counts):
        w = host(winners[b])
        assert np.array_equal(w[:n], host(cpu.voxel_winners(VS)[b])) and (w[n:] == -1).all(), b
    bounds = list(pc._dcount[0].group.bounds)
    caps = [t.shape[0] for t in pc._buf["points"]]
    gen = pc._generation
    assert pc.voxel_downsample_(VS) is pc
    cpu.voxel_downsample_(VS)
    assert len(pc._dcount) == 2, "the thinning resolved a device-side count"
    assert pc._dcount[0].group.bounds == bounds, "the bounds change only when a read-back lands"
    assert [t.shape[0] for t in pc._buf["points"]] == caps and pc._generation > gen
    assert pc.last_pruned.is_cuda
    # ... and only now the comparison asks for the counts
    assert pc._tighten_counts() == cpu._n
    assert host(pc.last_pruned).tolist() == cpu.last_pruned.tolist() and all(0 < r < n for r, n in
                                                                             zip(cpu.last_pruned.tolist(), counts))
    assert host(pc._marks[:, :1]).tolist() == cpu._marks[:, :1].tolist(), "the marks are rewritten"
    for b, n in enumerate(cpu._n):
        for k in ("points", "normals", "colors", "features"):
            assert np.array_equal(bits(host(pc._buf[k][b][:n])), bits(cpu._buf[k][b][:n].numpy())), (b, k)
        # (the CPU path itself is pinned to restatement + restated prune by tests/test_voxel_cpu.py; once more here)
        keep = vr.voxel_keep(arrs[b][0], arrs[b][3], counts[b], VS)[0]
        want = pr.prune(*arrs[b], counts[b], None, keep, [counts[b] // 2], -1)
        assert want[4] == n and np.array_equal(bits(host(pc._buf["points"][b][:n])), bits(want[0]))
    # out of place: the source stays; a second pass removes nothing
    out = pc.voxel_downsample(4 * VS)
    assert out is not pc and pc._tighten_counts() == cpu._n and sum(out._n) < sum(cpu._n)
    pc.voxel_downsample_(VS)
    assert host(pc.last_pruned).tolist() == [0, 0] and pc._tighten_counts() == cpu._n


def test_thinning_a_taped_map_keeps_the_rows_on_the_tape(gs):
    P, C = fixture_data()
    n = 300
    Q = np.where(np.isfinite(P[:n]), P[:n], 0).astype(f32)
    Pg = dev(Q).requires_grad_(True)
    z = lambda c: dev(np.zeros((n, c), f32))   # noqa: E731
    pc = gs.Pointclouds([Pg], [z(3)], [z(3)], [dev(C[:n].reshape(-1, 1))])
    out = pc.voxel_downsample(VS)
    keep = vr.voxel_keep(Q, C[:n], n, VS)[0] != 0
    assert out._n == [int(keep.sum())] and 0 < keep.sum() < n
    out.points_list[0].sum().backward()
    assert np.array_equal(host(Pg.grad), np.repeat(keep[:, None], 3, 1).astype(f32))


def test_backward_of_a_render_taken_before_a_thinning_raises(gs):
    pc, _ = device_map(gs, (NROWS,), extra=0)
    K = np.array([[45.0, 0, 26.0, 0], [0, 45.0, 18.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
    pose = torch.eye(4, device="cuda").view(1, 1, 4, 4).clone().requires_grad_(True)
    stale = pc.render(dev(K).view(1, 1, 4, 4), pose, 37, 53, differentiable=True).depth_image.sum()
    pc.voxel_downsample_(VS)
    with pytest.raises(RuntimeError, match="changed in place"):
        stale.backward()


# ------------------------------------------------------------------------------------------ end to end
L_SEQ, SEQ_H, SEQ_W = 8, 60, 80
VOX = 2.0 ** -6
PRUNE = dict(prune_min_confidence=0.004, prune_min_age=2, prune_every=2)
CARVE = dict(carve_margin=0.05, carve_window=1)


@pytest.fixture(scope="module")
def seq():
    from gradslam_amd.datasets.synthetic import make_sequence
    return make_sequence(L_SEQ, SEQ_H, SEQ_W, seed=0, scene="wave")


def oracle_run(s, odom, every, full=False, marks=None):
    """the oracle loop with, after the map update of every `every`-th step, voxel_ref.thin_map's rule applied as a prune
    by the restated keep mask (which also rewrites the epoch marks); with `full`, the restated carve before it and the
    restated pruning schedule after it: carve -> thin -> prune"""
    from tests import carve_ref as cr
    Kc = s["intrinsics"][0]
    marks, removed = [] if marks is None else marks, []

    def apply(m, keep):
        out = pr.prune(m.points, m.normals, m.colors, m.ccounts, len(m), None, keep, marks, -1)
        m.points, m.normals, m.colors, m.ccounts = out[:4]
        marks[:] = out[6]
        return out[5]

    def per_frame(i, m, pose):
        if full:
            apply(m, cr.free_space(m.points, len(m), [s["depths"][i]], [pose], Kc, 0.05, 1, 1)[1])
        if (i + 1) % every == 0:
            removed.append(apply(m, vr.voxel_keep(m.points, m.ccounts, len(m), VOX)[0]))
        else:
            removed.append(None)
        if not full:
            return
        if (i + 1) % PRUNE["prune_every"] == 0 and len(marks) >= PRUNE["prune_min_age"]:
            out = pr.prune(m.points, m.normals, m.colors, m.ccounts, len(m), PRUNE["prune_min_confidence"], None, marks,
                           len(marks) - PRUNE["prune_min_age"])
            m.points, m.normals, m.colors, m.ccounts = out[:4]
            marks[:] = out[6]
        marks.append(len(m))

    m, poses = oslam.run_sequence(s["colors"], s["depths"], Kc, s["poses"], odom=odom, per_frame=per_frame)
    return m, poses, removed


_ORACLE = {}


def oracle(s, odom, every, full=False):
    key = (odom, every, full)
    if key not in _ORACLE:
        marks = []
        _ORACLE[key] = oracle_run(s, odom, every, full, marks) + (marks,)
    return _ORACLE[key]


def frames_of(gs, s, odom):
    poses = T(s["poses"][None].copy()).cuda()
    if odom != "gt":
        poses[:, 1:] = poses[:, :1]
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)


def step_loop(gs, slam, frames, odom, inplace=True):
    pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
    for i in range(L_SEQ):
        live = frames[:, i]
        pc, p = slam.step(pc, live, prev, inplace=inplace)
        prev = live if odom != "gt" else None
        rec.append(host(p[0, 0]))
    return pc, np.stack(rec)


def same_as_oracle(pc, poses, m, oposes, what):
    got = [host(x[0]) for x in (pc.points_list, pc.normals_list, pc.colors_list, pc.features_list)]
    assert got[0].shape == m.points.shape, (what, got[0].shape, m.points.shape)
    for name, a, b in zip(("points", "normals", "colors", "ccounts", "poses"), got + [poses],
                          (m.points, m.normals, m.colors, m.ccounts, oposes)):
        assert np.array_equal(bits(a), bits(b)), "%s %s: %d of %d differ" % (what, name, (a != b).sum(), a.size)


@pytest.mark.parametrize("every", [1, 3])
def test_thinning_slam_equals_the_thinning_oracle(gs, seq, every):
    m, oposes, removed, _ = oracle(seq, "gt", every)
    plain, _ = oslam.run_sequence(seq["colors"], seq["depths"], seq["intrinsics"][0], seq["poses"], odom="gt")
    print("oracle thinning every", every, "rows removed per step:", removed, "final", len(m), "unthinned", len(plain))
    assert sum(r for r in removed if r) > 1000 and len(m) < len(plain)
    slam = gs.slam.PointFusion(odom="gt", device="cuda", voxel_size=VOX, voxel_every=every)
    pc, poses = step_loop(gs, slam, frames_of(gs, seq, "gt"), "gt")
    assert len(pc._dcount) == 1, "the counts stay on the device through the thinning"
    assert pc._voxel_steps == L_SEQ
    same_as_oracle(pc, poses, m, oposes, "gt, every %d" % every)
    # forward, and out-of-place steps
    pc, poses = gs.slam.PointFusion(odom="gt", device="cuda", voxel_size=VOX, voxel_every=every)(frames_of(gs, seq, "gt"))
    same_as_oracle(pc, host(poses[0]), m, oposes, "forward, every %d" % every)
    pc, poses = step_loop(gs, slam, frames_of(gs, seq, "gt"), "gt", inplace=False)
    assert pc._voxel_steps == L_SEQ
    same_as_oracle(pc, poses, m, oposes, "out of place, every %d" % every)


def test_fast_path_thins_the_same(gs, seq):
    """gradICP odometry: the in-place loop takes the one-call fast path from the second frame on"""
    m, oposes, removed, _ = oracle(seq, "gradicp", 1)
    assert sum(removed) > 1000
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", voxel_size=VOX, voxel_every=1)
    pc, poses = step_loop(gs, slam, frames_of(gs, seq, "gradicp"), "gradicp")
    assert getattr(slam, "_step_plan", None) is not None, "the in-place loop must have taken the fast path"
    assert len(pc._dcount) == 1
    same_as_oracle(pc, poses, m, oposes, "fast path")


def test_order_is_carve_then_thin_then_prune(gs, seq):
    m, oposes, removed, marks = oracle(seq, "gradicp", 1, full=True)
    assert len(marks) == L_SEQ and marks[-1] == len(m) and sum(removed) > 1000
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda", voxel_size=VOX, voxel_every=1, **CARVE, **PRUNE)
    pc, poses = step_loop(gs, slam, frames_of(gs, seq, "gradicp"), "gradicp")
    assert pc._voxel_steps == pc._carve_steps == pc._prune_steps == L_SEQ
    assert host(pc._marks[0, :pc._n_marks]).tolist() == marks
    same_as_oracle(pc, poses, m, oposes, "carve + thin + prune")


def test_voxel_size_none_is_bit_equal_to_a_driver_built_without_the_argument(gs, seq):
    for odom in ("gt", "gradicp"):
        a, pa = step_loop(gs, gs.slam.PointFusion(odom=odom, device="cuda"), frames_of(gs, seq, odom), odom)
        b, pb = step_loop(gs, gs.slam.PointFusion(odom=odom, device="cuda", voxel_size=None, voxel_every=5),
                          frames_of(gs, seq, odom), odom)
        assert b._voxel_steps == 0 and b.last_pruned is None and np.array_equal(bits(pa), bits(pb))
        for x, y in zip((a.points_list, a.normals_list, a.colors_list, a.features_list),
                        (b.points_list, b.normals_list, b.colors_list, b.features_list)):
            assert np.array_equal(bits(host(x[0])), bits(host(y[0])))
    m, oposes = oslam.run_sequence(seq["colors"], seq["depths"], seq["intrinsics"][0], seq["poses"], odom="gradicp")
    same_as_oracle(b, pb, m, oposes, "voxel_size=None")


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from gradslam_amd.datasets.synthetic import make_sequence
odom, every = sys.argv[2], int(sys.argv[3])
s = make_sequence(8, 60, 80, seed=0, scene="wave")
T = torch.from_numpy
poses = T(s["poses"][None].copy()).cuda()
if odom != "gt":
    poses[:, 1:] = poses[:, :1]
frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
slam = gs.slam.PointFusion(odom=odom, device="cuda", voxel_size=2.0 ** -6, voxel_every=every)
pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
for i in range(8):
    live = frames[:, i]
    pc, p = slam.step(pc, live, prev, inplace=True)
    prev = live if odom != "gt" else None
    rec.append(p[0, 0].cpu().numpy())
assert getattr(slam, "_step_plan", None) is None, "GRADSLAM_HIP_FASTPATH=0 must keep the fast path out"
np.savez(sys.argv[1], poses=np.stack(rec), pts=pc.points_list[0].cpu().numpy(), nrm=pc.normals_list[0].cpu().numpy(),
         col=pc.colors_list[0].cpu().numpy(), cc=pc.features_list[0].cpu().numpy())
"""


@pytest.mark.parametrize("odom,every", [("gradicp", 1), ("gt", 3)])
def test_generic_path_thins_the_same(seq, tmp_path, odom, every):
    m, oposes, _, _ = oracle(seq, odom, every)
    out = str(tmp_path / "generic.npz")
    subprocess.run([sys.executable, "-c", _CHILD % REPO, out, odom, str(every)], check=True, timeout=600,
                   env=dict(os.environ, GRADSLAM_HIP_FASTPATH="0"))
    z = np.load(out)
    for name, a, b in (("points", z["pts"], m.points), ("normals", z["nrm"], m.normals), ("colors", z["col"], m.colors),
                       ("ccounts", z["cc"], m.ccounts), ("poses", z["poses"], oposes)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), "generic path " + name


# ------------------------------------------------------------------------------------------ the C entry point
@pytest.mark.parametrize("case", sorted(vc.INVALID))
def test_entry_point_rejects_before_any_hip_call(case):
    vc.check_refusal(_C, case)


def test_entry_point_checks_every_sequence_and_sizes_the_table():
    vc.check_refusals_of_the_batch(_C)
