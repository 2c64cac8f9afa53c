"""The three spellings of a map -- plain tuples, ops.MapRows, the Pointclouds methods -- are one call: the same bits out of
render, free-space, voxel and prune.  B = 3 maps of 37, 5 and 0 live rows in 64-row buffers, every device count below its
host bound, the middle map's points a strided view (a converted copy is held while a later sequence's outputs are
allocated): the smallest shapes that cross a partial tile, an empty map and a batch with a held copy in the middle."""
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP, LIVE, SLACK, HW = 64, (37, 5, 0), 3, 8
VOXEL, MIN_CONF = 0.25, 0.5


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(11)
    bufs = []
    for b, n in enumerate(LIVE):
        P = torch.rand(CAP, 3, generator=g) * torch.tensor([0.8, 0.8, 1.0]) + torch.tensor([-0.4, -0.4, 1.0])
        P[n:] = 50.0 + torch.arange(CAP - n).unsqueeze(1)   # (rows behind the count: finite, far away, never read)
        N = torch.nn.functional.normalize(torch.rand(CAP, 3, generator=g) - 0.5, dim=1)
        row = [P, N, torch.rand(CAP, 3, generator=g), torch.rand(CAP, 1, generator=g)]
        row = [t.to(DEV) for t in row]
        if b == 1:
            wide = torch.zeros(2 * CAP, 3, device=DEV)
            wide[::2] = row[0]
            row[0] = wide[::2]
            assert not row[0].is_contiguous()
        bufs.append(row)
    counts = torch.tensor(LIVE, dtype=torch.int64, device=DEV)
    tuples = [tuple(bufs[b]) + (LIVE[b] + SLACK, counts[b:b + 1]) for b in range(3)]
    K = torch.tensor([[HW, 0, HW / 2, 0], [0, HW, HW / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=DEV)
    K = K.expand(3, 4, 4).contiguous()
    poses = torch.eye(4, device=DEV).expand(3, 1, 4, 4).contiguous()
    # mostly behind every point (a see-through needs its whole window there), some holes, some pixels in front
    depth = torch.tensor([0.0, 1.2, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0])[torch.randint(0, 8, (3, 1, HW, HW), generator=g)]
    depth = depth.to(DEV)
    # the container over the same buffers and device counts; its host bounds start above every count and follow its own
    # read-backs from there
    pc = gs.Pointclouds(device=DEV)
    pc._init_empty_batch(3, 1)
    for i, k in enumerate(("points", "normals", "colors", "features")):
        pc._buf[k] = [bufs[b][i] for b in range(3)]
    pc._set_counts_dev(counts.clone(), max(LIVE) + SLACK)
    return dict(tuples=tuples, rows=[ops.MapRows(*t) for t in tuples], K=K, poses=poses, depth=depth, pc=pc)


def _live_prefix(x, y, live, fill):
    """x and y are (bound,) outputs of one map under two host bounds (the container's follows its own read-backs): the same
    bits as far as both go, which covers the live rows, and the fill of rows at or beyond the device count after that"""
    n = min(x.shape[0], y.shape[0])
    assert n >= live
    _same(x[:n], y[:n])
    assert bool((x[live:] == fill).all()) and bool((y[live:] == fill).all())


def test_render(scene):
    a = ops.render_map_batch(scene["tuples"], scene["poses"], scene["K"], HW, HW)
    b = ops.render_map_batch(scene["rows"], scene["poses"], scene["K"], HW, HW)
    frames, extra = scene["pc"].render(scene["K"].unsqueeze(1), scene["poses"], HW, HW, return_extras=True)
    c = (frames.depth_image, frames.rgb_image, extra["normal"], extra["confidence"], extra["index"])
    for x, y, z in zip(a, b, c):
        _same(x, y)
        _same(x, z)
    assert int((a.index[0] >= 0).sum()) > 0 and int((a.index[1] >= 0).sum()) > 0 and bool((a.index[2] == -1).all())
    assert int(a.index.max()) < max(LIVE)


def test_free_space(scene):
    a = ops.free_space_batch(scene["tuples"], scene["depth"], scene["poses"], scene["K"])
    b = ops.free_space_batch(scene["rows"], scene["depth"], scene["poses"], scene["K"])
    frames = gs.RGBDImages(torch.zeros(3, 1, HW, HW, 3, device=DEV), scene["depth"].unsqueeze(-1),
                           scene["K"].unsqueeze(1), scene["poses"])
    c = scene["pc"].free_space_violations(frames)
    for s in range(3):
        assert a.violations[s].shape == (LIVE[s] + SLACK,)
        _same(a.violations[s], b.violations[s])
        _same(a.keep[s], b.keep[s])
        _live_prefix(a.violations[s], c[s], LIVE[s], 0)
    assert int(a.violations[0].sum()) > 0


def test_voxel_keep(scene):
    a = ops.voxel_keep_batch(scene["tuples"], VOXEL)
    b = ops.voxel_keep_batch(scene["rows"], VOXEL)
    c = scene["pc"].voxel_winners(VOXEL)
    _same(a.unplaced, b.unplaced)
    for s in range(3):
        assert a.winner[s].shape == (LIVE[s] + SLACK,)
        _same(a.keep[s], b.keep[s])
        _same(a.winner[s], b.winner[s])
        _live_prefix(a.winner[s], c[s], LIVE[s], -1)
    assert 0 < int(a.keep[0].sum()) < LIVE[0]


def test_prune(scene):
    a = ops.prune_map_batch(scene["tuples"], min_confidence=MIN_CONF)
    b = ops.prune_map_batch(scene["rows"], min_confidence=MIN_CONF)
    _same(a.counts, b.counts)
    _same(a.removed, b.removed)
    counts = a.counts.tolist()
    assert 0 < counts[0] < LIVE[0] and counts[2] == 0 and [c + r for c, r in zip(counts, a.removed.tolist())] == list(LIVE)
    # last: it rewrites the container (new buffers; the module's tuples keep the old ones)
    pc = scene["pc"].prune_(MIN_CONF)
    assert pc._n == counts
    _same(a.removed, pc.last_pruned)
    for s in range(3):
        for i, k in enumerate(("points", "normals", "colors", "features")):
            _same(a.maps[s][i][:counts[s]], b.maps[s][i][:counts[s]])
            _same(a.maps[s][i][:counts[s]], pc._buf[k][s][:counts[s]])
