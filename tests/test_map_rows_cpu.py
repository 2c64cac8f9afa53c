"""ops.MapRows and the host-side marshalling every batched map pass shares (_map_rows, _map_view, _seq_outs, _rows_bar):
the bound rule, the tuple forms, the pointers a gs_map_view gets and who keeps a converted copy alive.  CPU tensors only:
none of the helpers touches the device or the library."""
import pytest
import torch

from gradslam_amd import _C, ops

ROWS = 12


def _map(n_bound=None, n_dev=None, **kw):
    g = torch.Generator().manual_seed(3)
    bufs = dict(points=torch.rand(ROWS, 3, generator=g), normals=torch.rand(ROWS, 3, generator=g),
                colors=torch.rand(ROWS, 3, generator=g), features=torch.rand(ROWS, 1, generator=g))
    bufs.update(kw)
    return ops.MapRows(n_bound=n_bound, n_dev=n_dev, **bufs)


@pytest.mark.parametrize("given,want", [(None, ROWS), (ROWS + 5, ROWS), (ROWS, ROWS), (ROWS - 1, ROWS - 1), (5, 5), (0, 0)])
def test_bound_resolves_against_the_rows(given, want):
    m = ops._map_rows(_map(given))
    assert m.n_bound == want and type(m.n_bound) is int
    v = ops._map_view(m)
    assert v.n_bound == want and v.capacity == ROWS


def test_negative_bound_is_left_to_the_entry():
    assert ops._map_rows(_map(-3)).n_bound == -3   # (carve / voxel refuse it, the projective ICP clamps it, ...)


def test_three_spellings_give_one_object():
    src = _map(7, torch.tensor([6]))
    a = ops._map_rows(src, read=("points", "normals"), four_ok=True)
    b = ops._map_rows(tuple(src), read=("points", "normals"), four_ok=True)
    c = ops._map_rows((src.points, src.normals, src.n_bound, src.n_dev), read=("points", "normals"), four_ok=True)
    assert isinstance(a, ops.MapRows)
    for other in (b, c):
        assert type(other) is ops.MapRows and len(other) == 6
        assert all(x is y for x, y in zip(a, other))
    assert a.points is src.points and a.normals is src.normals and a.colors is None and a.features is None
    assert a.n_bound == 7 and a.n_dev is src.n_dev
    # a list entry is a tuple entry
    assert all(x is y for x, y in zip(ops._map_rows(list(src)), ops._map_rows(src)))


def test_short_form_only_where_an_entry_allows_it():
    src = _map(7)
    short = (src.points, src.normals, 7, None)
    # the six-field entries index the fifth field of what they are given, as before: IndexError
    with pytest.raises(IndexError):
        ops._map_rows(short)
    with pytest.raises(IndexError):
        ops._map_rows(short, read=("points",), four_ok=False)
    # ... and the two entries that name the form in their refusal still do, before anything is converted
    K = torch.eye(4).unsqueeze(0)
    with pytest.raises(ValueError, match=r"free_space: maps\[0\] must be \(points, normals, colors, ccounts, n_bound, n_dev\)"):
        ops.free_space_batch([short], torch.ones(1, 1, 4, 4), K.unsqueeze(0), K)
    with pytest.raises(ValueError, match=r"voxel_keep: maps\[0\] must be \(points, normals, colors, features, n_bound, n_dev\)"):
        ops.voxel_keep_batch([short], 0.1)


def test_attributes_not_read_or_absent_are_null():
    m = ops._map_rows(_map(colors=None), read=("points", "features"))
    assert m.normals is None and m.colors is None and m.features is not None
    v = ops._map_view(m)
    assert v.points == m.points.data_ptr() and v.ccounts == m.features.data_ptr()
    assert not v.normals and not v.colors          # (a NULL c_void_p field reads None)
    assert not v.n_dev
    n_dev = torch.tensor([4])
    v = ops._map_view(ops._map_rows(_map(n_dev=n_dev)))
    assert v.n_dev == n_dev.data_ptr() and v.normals and v.colors and v.ccounts
    assert isinstance(v, _C.MapView)
    # the spelled-out form of a caller that fills a descriptor by hand: four buffers, then capacity, bound, device count
    src = _map()
    w = ops._map_view(list(src[:4]), ROWS - 2, 5, n_dev[0:])
    assert (w.points, w.normals, w.colors, w.ccounts) == tuple(t.data_ptr() for t in src[:4])
    assert (w.capacity, w.n_bound, w.n_dev) == (ROWS - 2, 5, n_dev.data_ptr())


def test_contiguous_float32_passes_through_by_identity():
    src = _map()
    m = ops._map_rows(src)
    assert all(m[i] is src[i] for i in range(4))
    v = ops._map_view(m)
    assert (v.points, v.normals, v.colors, v.ccounts) == tuple(t.data_ptr() for t in src[:4])
    # off the tape, same storage
    p = src.points.clone().requires_grad_(True)
    m = ops._map_rows(src._replace(points=p))
    assert not m.points.requires_grad and m.points.data_ptr() == p.data_ptr()


@pytest.mark.parametrize("kind", ["strided", "float64", "float64 on the tape"])
def test_converted_copy_is_held_by_the_result(kind):
    if kind == "strided":
        given = torch.rand(2 * ROWS, 3)[::2]
        assert not given.is_contiguous()
    else:
        given = torch.rand(ROWS, 3, dtype=torch.float64, requires_grad=kind.endswith("tape"))
    m = ops._map_rows(_map(points=given, n_bound=ROWS + 1))
    assert m.points is not given and m.points.dtype == torch.float32 and m.points.is_contiguous()
    assert not m.points.requires_grad and m.points.data_ptr() != given.data_ptr()
    assert torch.equal(m.points, given.detach().to(torch.float32))
    v = ops._map_view(m)
    assert v.points == m.points.data_ptr() and v.capacity == ROWS and v.n_bound == ROWS


# ------------------------------------------------------------------------------------------ _seq_outs
SPEC = (("violations", torch.int32), ("keep", torch.uint8))


def test_seq_outs_allocates_or_takes():
    a, b = ops._seq_outs("free_space", None, SPEC, 0, 5, torch.device("cpu"))
    assert a.dtype == torch.int32 and b.dtype == torch.uint8 and a.shape == b.shape == (5,)
    v, k = torch.empty(5, dtype=torch.int32), torch.empty(5, dtype=torch.uint8)
    got = ops._seq_outs("free_space", ([None, v], [None, k]), SPEC, 1, 5, torch.device("cpu"))
    assert got[0] is v and got[1] is k
    # a missing list, or a None entry of one: that output is not produced
    assert ops._seq_outs("free_space", (None, [k]), SPEC, 0, 5, None) == [None, k]
    got = ops._seq_outs("free_space", ([v], [None]), SPEC, 0, 5, None)
    assert got[0] is v and got[1] is None


@pytest.mark.parametrize("out,message", [
    ((None, None), "free_space: out must ask for violations or keep (or both) of every map"),
    (([None], [None]), "free_space: out must ask for violations or keep (or both) of every map"),
    (([torch.empty(5, dtype=torch.int64)], None),
     "free_space: out.violations[0] must be a contiguous int32 tensor of shape (5,)"),
    (([torch.empty(4, dtype=torch.int32)], None),
     "free_space: out.violations[0] must be a contiguous int32 tensor of shape (5,)"),
    ((None, [torch.empty(10, dtype=torch.uint8)[::2]]),
     "free_space: out.keep[0] must be a contiguous uint8 tensor of shape (5,)"),
    ((None, [[0] * 5]), "free_space: out.keep[0] must be a contiguous uint8 tensor of shape (5,)"),
])
def test_seq_outs_refusals(out, message):
    with pytest.raises(ValueError) as e:
        ops._seq_outs("free_space", out, SPEC, 0, 5, None)
    assert str(e.value) == message
    other = (("keep", torch.uint8), ("winner", torch.int64))
    with pytest.raises(ValueError, match=r"voxel_keep: out must ask for keep or winner \(or both\) of every map"):
        ops._seq_outs("voxel_keep", (None, None), other, 0, 5, None)


# ------------------------------------------------------------------------------------------ _rows_bar
@pytest.mark.parametrize("n_bound", [0, 1, ROWS - 1, ROWS])
@pytest.mark.parametrize("width", [3, 1])
def test_rows_bar_zeroes_the_tail_only(monkeypatch, n_bound, width):
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real(*a, **k).fill_(7.0))   # what "uninitialised" holds here
    g = ops._rows_bar(ROWS, width, n_bound, torch.device("cpu"))
    assert g.shape == (ROWS, width) and g.dtype == torch.float32 and g.is_contiguous()
    assert bool((g[:n_bound] == 7.0).all()) and bool((g[n_bound:] == 0.0).all())


# ------------------------------------------------------------------------------------------ the container's builder
def test_pointclouds_builds_the_list():
    from gradslam_amd import Pointclouds
    pts = [torch.rand(n, 3) for n in (5, 9)]
    pc = Pointclouds(points=pts, normals=[p.clone() for p in pts], features=[torch.rand(p.shape[0], 1) for p in pts])
    maps = pc._map_rows()
    assert [type(m) for m in maps] == [ops.MapRows] * 2
    for b, m in enumerate(maps):
        assert m.points is pc._buf["points"][b] and m.normals is pc._buf["normals"][b]
        assert m.colors is None and m.features is pc._buf["features"][b]
        assert (m.n_bound, m.n_dev) == (pts[b].shape[0], None)
    only = pc._map_rows(("points",))
    assert all(m.points is pc._buf["points"][b] and m[1:4] == (None, None, None) for b, m in enumerate(only))
    outs = pc._row_outs(maps, torch.uint8, True)
    assert [tuple(t.shape) for t in outs] == [(5,), (9,)] and all(t.dtype == torch.uint8 for t in outs)
    assert pc._row_outs(maps, torch.uint8, False) == [None, None]
    assert Pointclouds()._map_rows() == []
