"""GPU tests of the render backward (gs_render.hip: gs_render_map_backward_dc_f32 -> ops.RenderMapFunction ->
ops.render_map(differentiable=True) -> Pointclouds.render(differentiable=True) -> metrics.render_loss) against the
float64 NumPy adjoint of tests/render_grad_ref.py on the cases of tests/render_backward_cases.py.

Bounds.  points_bar, normals_bar and poses_bar: `rel_err` (largest error over all elements relative to the largest
reference element) within backward_cases.kernel_bound(gap), gap = the committed CPU gap of the case and output (float32
against float64 NumPy); an output whose reference is zero must be exactly zero.  colors_bar and ccounts_bar are sums of
copies (at most 25 pixels x 9 views, added in float64 and rounded once per launch of 4 views): kernel_bound(0), the
floor of FLOOR_ULPS float32 ulps of the largest element.  Everything else is compared for equal bits.  No bound comes
from the kernel's output.  Every case first asserts on its own input (render_backward_cases.claims, from the CPU
restatement of the forward) that it exercises what it claims, and that the HIP index image is the restated one."""
import warnings

import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import render_backward_cases as rc
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

T = torch.from_numpy
NAMES = ("points_bar", "normals_bar", "colors_bar", "ccounts_bar", "poses_bar")


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


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


def upstream(c, nan_empty=False):
    """the case's upstream adjoints shaped like the images of ops.render_map (None where the case has none)"""
    out = []
    for a, tail in ((c.zb, (1,)), (c.cb, (3,)), (c.ob, (3,)), (c.fb, (1,))):
        if a is None:
            out.append(None)
            continue
        a = a.reshape(c.index.shape + tail).copy()
        if nan_empty:
            a[c.index < 0] = np.nan
        out.append(dev(a))
    return out


def backward_through(images, ups):
    pairs = [(img, up) for img, up in zip(images, ups) if up is not None]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])


def hip_grads(ops, c, ups=None, arrays=None, n_dev=None, poses=None):
    """gradients of sum(image * upstream) through ops.render_map(differentiable=True): the five outputs as numpy arrays
    (+ K.grad, which must be None)"""
    arrays = arrays if arrays is not None else (c.points, c.normals, c.colors, c.ccounts)
    leaves = [dev(a).requires_grad_(True) for a in arrays]
    P = dev(c.poses if poses is None else poses).requires_grad_(True)
    K = dev(c.K).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # differentiable=True emits no warning
        r = ops.render_map(*leaves, P, K, c.H, c.W, n_dev=n_dev, differentiable=True, **c.kw)
    assert r.depth.requires_grad and r.color.requires_grad and r.normal.requires_grad and r.confidence.requires_grad
    assert not r.index.requires_grad and r.index.dtype == torch.int64
    if poses is None:
        assert np.array_equal(host(r.index), c.index), "the HIP winners are the restated ones"
        assert np.array_equal(host(r.depth)[..., 0], c.depth)
    backward_through((r.depth, r.color, r.normal, r.confidence), upstream(c) if ups is None else ups)
    assert K.grad is None
    return [host(t.grad) for t in leaves] + [host(P.grad)]


def within(c, got, ref=None, rows=None):
    """the per-element check of one case; rows: compare the first `rows` rows of the row outputs, the rest is zero"""
    ref = rc.reference(c) if ref is None else ref
    gap = dict(zip(rc.OUTPUTS, rc.GAP[c.name]))
    for name, g, r in zip(NAMES, got, ref):
        g = g.reshape(g.shape[0], -1) if name != "poses_bar" else g
        r = r.reshape(r.shape[0], -1) if name != "poses_bar" else r
        if rows is not None and name != "poses_bar":
            assert not g[rows:].any(), "%s: %s is not zero beyond the count" % (c.name, name)
            g = g[:rows]
        assert g.shape == r.shape and g.dtype == np.float32, (c.name, name, g.shape, r.shape, g.dtype)
        assert np.isfinite(g).all(), (c.name, name)
        if not np.abs(r).max() > 0:
            assert not g.any(), "%s: %s must be exactly zero" % (c.name, name)
            continue
        bound = bc.kernel_bound(gap[name]) if name in gap else bc.kernel_bound(0.0)
        err = bc.rel_err(g, r)
        print("%-12s %-11s err %.2e bound %.2e" % (c.name, name, err, bound))
        assert err <= bound, (c.name, name, err, bound)
    # by bits: rows that win nothing, the bottom row of the pose adjoint
    won = np.zeros(len(c.points), bool)
    won[c.index[c.index >= 0]] = True
    for name, g in zip(NAMES[:4], got[:4]):
        assert not g[:len(c.points)][~won].any(), "%s: %s of a row that wins nothing" % (c.name, name)
    assert not got[4][:, 3].any(), "%s: bottom row of poses_bar" % c.name


@pytest.mark.parametrize("name", [n for n in sorted(rc.CASES) if n not in ("ragged_9001", "loss6")])
def test_backward_equals_float64_adjoint(ops, name):
    c = rc.build(name)
    rc.claims(c)
    got = hip_grads(ops, c)
    within(c, got)
    again = hip_grads(ops, c)
    for n_, a, b in zip(NAMES, got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: two identical calls differ in %s" % (name, n_)


@pytest.mark.parametrize("name", ["r0_seq", "big_r0"])
def test_copies_are_exact_at_one_view_and_radius_zero(ops, name):
    c = rc.build(name)
    assert c.index.shape[0] == 1 and c.kw.get("radius", 0) == 0
    hit = c.index >= 0
    assert np.bincount(c.index[hit]).max() == 1, "at radius 0 a row wins at most one pixel"
    got = hip_grads(ops, c)
    want_c, want_f = np.zeros_like(c.colors), np.zeros_like(c.ccounts).reshape(-1)
    want_c[c.index[hit]] = c.cb[hit]
    want_f[c.index[hit]] = c.fb[hit]
    assert np.array_equal(got[2].view(np.uint32), want_c.view(np.uint32))
    assert np.array_equal(got[3].reshape(-1).view(np.uint32), want_f.view(np.uint32))


def test_each_view_of_nine_equals_its_single_view_call(ops):
    c = rc.build("views9")
    assert c.index.shape[0] == 9
    got = hip_grads(ops, c)
    ups = upstream(c)
    for v in range(9):
        one = hip_grads(ops, c, ups=[u[v:v + 1] for u in ups], poses=c.poses[v:v + 1])
        assert np.array_equal(one[4][0].view(np.uint32), got[4][v].view(np.uint32)), "poses_bar of view %d" % v


@pytest.mark.parametrize("name", ["r2_off", "views9"])
def test_nan_upstream_at_empty_pixels_changes_nothing(ops, name):
    c = rc.build(name)
    assert (c.index < 0).any()
    clean = hip_grads(ops, c)
    dirty = hip_grads(ops, c, ups=upstream(c, nan_empty=True))
    for n_, a, b in zip(NAMES, clean, dirty):
        assert np.isfinite(b).all(), (name, n_)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, n_)


def test_device_count_below_the_capacity(ops):
    c = rc.build("r1_off")
    n, cap = len(c.points), len(c.points) + 5000
    pose = c.poses[0]
    # filler rows behind the count: a plane 0.3 m in front of the camera (it would win every pixel it covers)
    rng = np.random.default_rng(3)
    cam = np.stack([rng.uniform(-0.1, 0.1, cap - n), rng.uniform(-0.1, 0.1, cap - n), np.full(cap - n, 0.3)], -1)
    filler = (cam @ pose[:3, :3].T.astype(np.float64) + pose[:3, 3]).astype(np.float32)
    arrays = [np.concatenate([a, f]) for a, f in (
        (c.points, filler), (c.normals, np.tile(np.float32([[0, 0, -1]]), (cap - n, 1))),
        (c.colors, np.full((cap - n, 3), 255, np.float32)), (c.ccounts, np.full((cap - n, 1), 50, np.float32)))]
    whole = rr.render(*arrays, pose, c.K, c.H, c.W, **c.kw)
    assert (whole.index >= n).sum() > 100, "the filler would show if it were counted in"
    got = hip_grads(ops, c, arrays=arrays, n_dev=torch.tensor([n], dtype=torch.int64, device="cuda"))
    assert got[0].shape == (cap, 3) and got[3].shape == (cap, 1)
    within(c, got, rows=n)
    exact = hip_grads(ops, c)
    for n_, a, b in zip(NAMES, got, exact):
        assert np.array_equal(a[:n].view(np.uint32) if n_ != "poses_bar" else a.view(np.uint32), b.view(np.uint32)), n_


def test_batch_of_two_with_ragged_counts(ops):
    c0, c1 = rc.build("views3"), rc.build("ragged_9001")
    rc.claims(c0)
    rc.claims(c1)
    assert c0.kw == c1.kw and c0.index.shape == c1.index.shape
    s, m = rc.scene("small")
    n1 = len(c1.points)
    assert n1 == 9001 < len(m)
    full = [np.ascontiguousarray(getattr(m, k), np.float32) for k in ("points", "normals", "colors", "ccounts")]
    la, lb = [dev(a).requires_grad_(True) for a in full], [dev(a).requires_grad_(True) for a in full]
    maps = [tuple(la) + (None, None), tuple(lb) + (len(m), torch.tensor([n1], dtype=torch.int64, device="cuda"))]
    P = dev(np.stack([c0.poses, c1.poses])).requires_grad_(True)
    K = dev(np.stack([c0.K, c1.K])).requires_grad_(True)
    r = ops.render_map_batch(maps, P, K, c0.H, c0.W, differentiable=True, **c0.kw)
    assert tuple(r.depth.shape) == (2, 3, c0.H, c0.W, 1) and tuple(r.index.shape) == (2, 3, c0.H, c0.W)
    assert np.array_equal(host(r.index[0]), c0.index) and np.array_equal(host(r.index[1]), c1.index)
    ups = [torch.stack([a, b]) for a, b in zip(upstream(c0), upstream(c1))]
    backward_through((r.depth, r.color, r.normal, r.confidence), ups)
    assert K.grad is None
    within(c0, [host(t.grad) for t in la] + [host(P.grad[0])])
    within(c1, [host(t.grad) for t in lb] + [host(P.grad[1])], rows=n1)
    # ... and equal bits with the single calls
    single = hip_grads(ops, c0)
    for n_, a, b in zip(NAMES, [host(t.grad) for t in la] + [host(P.grad[0])], single):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n_


def _bits_equal(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def test_entry_point_serves_two_ragged_sequences_in_one_call(ops):
    """gs_render_map_backward_dc_f32 with B = 2 in ONE call (ops.render_map_backward_batch): 9 views (three launches),
    sequence 0 the whole map, sequence 1 the same buffers with a host bound of 12 000 rows and a device count of 9 001
    (fewer blocks than sequence 0: its surplus blocks leave at once).  Equal bits with the two single-sequence calls,
    and sequence 0 within the bound of its case."""
    c = rc.build("views9")
    rc.claims(c)
    s, m = rc.scene("small")
    rows, bound1, n1 = len(m), 12000, 9001
    full = [dev(np.ascontiguousarray(getattr(m, k), np.float32)) for k in ("points", "normals", "colors", "ccounts")]
    n_dev = torch.tensor([n1], dtype=torch.int64, device="cuda")
    poses = dev(np.stack([c.poses, c.poses[::-1]]))
    K = dev(np.stack([c.K, rc.scaled_K(c.K, 0.9)]))
    H, W, radius = c.H, c.W, c.kw["radius"]
    fwd = ops.render_map_batch([tuple(full) + (None, None), tuple(full) + (bound1, n_dev)], poses, K, H, W, radius=radius)
    assert np.array_equal(host(fwd.index[0]), c.index)
    assert int(fwd.index[1].max()) < n1 and bool((fwd.index[1] >= 0).any())
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    ups = [torch.stack([u, torch.randn(u.shape, generator=g, device="cuda")]) for u in upstream(c)]
    maps = [(full[0], full[1], None, None), (full[0], full[1], bound1, n_dev)]
    both, T_both = ops.render_map_backward_batch(maps, poses, K, fwd.index, ups, H, W, radius)
    again, T_again = ops.render_map_backward_batch(maps, poses, K, fwd.index, ups, H, W, radius)
    _bits_equal(T_both, T_again, "poses_bar of two identical calls")
    assert tuple(T_both.shape) == (2, 9, 4, 4)
    for b in range(2):
        one, T_one = ops.render_map_backward_batch(maps[b:b + 1], poses[b:b + 1], K[b:b + 1], fwd.index[b:b + 1],
                                                   [u[b:b + 1] for u in ups], H, W, radius)
        _bits_equal(T_both[b], T_one[0], "poses_bar of sequence %d" % b)
        for name, x, y, z in zip(NAMES, both[b], one[0], again[b]):
            assert tuple(x.shape) == (rows, 1 if name == "ccounts_bar" else 3)
            _bits_equal(x, y, "%s of sequence %d: one call of two against a call of its own" % (name, b))
            _bits_equal(x, z, "%s of sequence %d: two identical calls" % (name, b))
    for x in both[1]:
        assert not bool(x[n1:].any()), "rows beyond the device count (and beyond the host bound) are zero"
        assert bool(x[:n1].any())
    within(c, [host(x) for x in both[0]] + [host(T_both[0])])
    # sequence 1 on an exact-size copy of its 9 001 rows: the same bits
    cut = [t[:n1].clone() for t in full[:2]]
    exact, T_exact = ops.render_map_backward_batch([(cut[0], cut[1], None, None)], poses[1:], K[1:], fwd.index[1:],
                                                   [u[1:] for u in ups], H, W, radius)
    _bits_equal(T_both[1], T_exact[0], "poses_bar: device count against exact size")
    for x, y in zip(both[1], exact[0]):
        _bits_equal(x[:n1], y, "device count against exact size")


@pytest.mark.parametrize("name", ["only_z", "only_c", "only_o", "only_f"])
def test_null_upstream_images_and_null_outputs(ops, name):
    """the entry point with NULL for every upstream image the case lacks (and NULL normals where no term reads them),
    with all outputs and with the pose adjoint alone"""
    c = rc.build(name)
    ups = upstream(c)
    assert sum(u is not None for u in ups) == 1
    P, N = dev(c.points), (dev(c.normals) if c.ob is not None else None)
    fwd = ops.render_map(P, dev(c.normals), dev(c.colors), dev(c.ccounts), dev(c.poses), dev(c.K), c.H, c.W, **c.kw)
    assert np.array_equal(host(fwd.index), c.index)
    args = ([(P, N, None, None)], dev(c.poses[None]), dev(c.K[None]), fwd.index.unsqueeze(0),
            [None if u is None else u.unsqueeze(0) for u in ups], c.H, c.W, c.kw["radius"])
    rows_out, T_bar = ops.render_map_backward_batch(*args)
    within(c, [host(x) for x in rows_out[0]] + [host(T_bar[0])])
    only_pose, T_only = ops.render_map_backward_batch(*args, want=(False, False, False, False, True))
    assert all(x is None for x in only_pose[0])
    _bits_equal(T_only, T_bar, "poses_bar with NULL row outputs")
    no_pose, T_none = ops.render_map_backward_batch(*args, want=(True, True, True, True, False))
    assert T_none is None
    for x, y in zip(no_pose[0], rows_out[0]):
        _bits_equal(x, y, "row outputs with NULL poses_bar")
    # through autograd the unused images arrive as None (not as zero images): the same bits
    got = hip_grads(ops, c)
    for name_, a, b in zip(NAMES, got, [host(x) for x in rows_out[0]] + [host(T_bar[0])]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name_


def test_backward_after_an_in_place_step_raises(gs):
    from gradslam_amd.datasets.synthetic import make_sequence
    L, H, W = 4, 96, 128
    s = make_sequence(L, H, W, seed=7)
    poses = T(s["poses"][None]).cuda()
    poses[:, 1:] = poses[:, :1]
    frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
    pc, prev, stale = gs.Pointclouds(device="cuda"), None, None
    for i in range(L):
        live = frames[:, i]
        with torch.no_grad():
            pc, p = slam.step(pc, live, prev, inplace=True)
        prev = live
        if i == L - 2:
            view = p.detach().clone().requires_grad_(True)
            fresh = pc.render(frames.intrinsics, view, H, W, differentiable=True).depth_image.sum()
            fresh.backward()   # before the next step: fine
            assert bool(view.grad.any())
            stale = pc.render(frames.intrinsics, view, H, W, differentiable=True).depth_image.sum()
    with pytest.raises(RuntimeError, match="changed in place"):
        stale.backward()


def test_interface(ops):
    c = rc.build("r0_seq")
    args = [dev(a) for a in (c.points, c.normals, c.colors, c.ccounts)]
    p = dev(c.points).requires_grad_(True)
    ref = ops.render_map(*args, dev(c.poses), dev(c.K), c.H, c.W)
    # the default still warns and still detaches
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        r = ops.render_map(p, *args[1:], dev(c.poses), dev(c.K), c.H, c.W)
    assert not r.depth.requires_grad and not r.color.requires_grad and torch.equal(r.depth, ref.depth)
    # differentiable=True: no warning, same images, out= refused
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d = ops.render_map(p, *args[1:], dev(c.poses), dev(c.K), c.H, c.W, differentiable=True)
    for a, b in zip(d, ref):
        assert torch.equal(a.detach(), b)
    assert d.depth.requires_grad and not d.index.requires_grad
    out = tuple(torch.empty_like(t) for t in ref)
    with pytest.raises(ValueError, match="out="):
        ops.render_map(p, *args[1:], dev(c.poses), dev(c.K), c.H, c.W, differentiable=True, out=out)
    with pytest.raises(ValueError, match="out="):
        ops.render_map_batch([tuple(args) + (None, None)], dev(c.poses[None]), dev(c.K[None]), c.H, c.W,
                             differentiable=True, out=tuple(t.unsqueeze(0) for t in out))
    # only the inputs that require grad get one; a loss on the depth alone leaves the colours at exact zero
    d.depth.sum().backward()
    assert p.grad is not None and bool(p.grad.any())
    c_leaf = dev(c.colors).requires_grad_(True)
    d2 = ops.render_map(args[0], args[1], c_leaf, args[3], dev(c.poses), dev(c.K), c.H, c.W, differentiable=True)
    d2.depth.sum().backward()
    assert c_leaf.grad is not None and not bool(c_leaf.grad.any())


def _frames(gs, s, poses=None, depths=None):
    return gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None] if depths is None else depths[None]).cuda(),
                         T(s["intrinsics"][None]).cuda(), T(s["poses"][None]).cuda() if poses is None else poses)


def test_pointclouds_render_differentiable(gs):
    c = rc.build("views3")
    s, m = rc.scene("small")
    frames = _frames(gs, s)
    pc, _ = gs.slam.PointFusion(odom="gt", device="cuda")(frames)
    n = len(m)
    bufs = [pc._buf[k][0] for k in ("points", "normals", "colors", "features")]
    assert bufs[0].shape[0] >= n and np.array_equal(host(bufs[0][:n]), c.points), "the HIP map is the oracle's map"
    for t in bufs:
        t.requires_grad_(True)
    poses = dev(c.poses[None]).requires_grad_(True)
    K = frames.intrinsics.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rendered, extras = pc.render(K, poses, c.H, c.W, return_extras=True, differentiable=True, **c.kw)
    assert isinstance(rendered, gs.RGBDImages) and rendered.shape == (1, 3, c.H, c.W)
    assert rendered.depth_image.requires_grad and rendered.rgb_image.requires_grad
    assert extras["normal"].requires_grad and extras["confidence"].requires_grad and not extras["index"].requires_grad
    assert np.array_equal(host(extras["index"][0]), c.index)
    backward_through((rendered.depth_image[0], rendered.rgb_image[0], extras["normal"][0], extras["confidence"][0]),
                     upstream(c))
    assert K.grad is None
    within(c, [host(t.grad) for t in bufs] + [host(poses.grad[0])], rows=n)
    # the default is unchanged: detached, with the warning
    with pytest.warns(RuntimeWarning, match="no backward kernel"):
        plain = pc.render(frames.intrinsics, poses, c.H, c.W, **c.kw)
    assert not plain.depth_image.requires_grad and torch.equal(plain.depth_image, rendered.depth_image.detach())


def test_differentiable_render_between_steps_with_device_counts(gs, ops):
    """PointFusion.step in place, a differentiable render and its backward between the steps: the counts stay on the
    device, the gradients equal (bit for bit) those of ops.render_map on an exact-size copy of the map, and the frame
    loop goes on."""
    from gradslam_amd.datasets.synthetic import make_sequence
    L, H, W = 5, 96, 128
    s = make_sequence(L, H, W, seed=7)
    poses = T(s["poses"][None]).cuda()
    poses[:, 1:] = poses[:, :1]
    frames = gs.RGBDImages(T(s["colors"][None]).cuda(), T(s["depths"][None]).cuda(), T(s["intrinsics"][None]).cuda(), poses)
    slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
    pc, prev, seen = gs.Pointclouds(device="cuda"), None, 0
    for i in range(L):
        live = frames[:, i]
        with torch.no_grad():
            pc, p = slam.step(pc, live, prev, inplace=True)
        prev = live
        if i < 2:
            continue
        assert pc._dcount, "the counts of an in-place map live on the device"
        dcount = dict(pc._dcount)
        view = p.detach().clone().requires_grad_(True)
        bufs = [pc._buf[k][0] for k in ("points", "normals", "colors", "features")]
        leaves = [t.detach().requires_grad_(True) for t in bufs]   # (same storage: nothing is copied)
        for k, t in zip(("points", "normals", "colors", "features"), leaves):
            pc._buf[k][0] = t
        r, extras = pc.render(frames.intrinsics, view, H, W, radius=1, return_extras=True, differentiable=True)
        assert pc._dcount == dcount, "the differentiable render resolved a device-side count"
        wz, wc = torch.randn_like(r.depth_image), torch.randn_like(r.rgb_image)
        wo, wf = torch.randn_like(extras["normal"]), torch.randn_like(extras["confidence"])
        torch.autograd.backward([r.depth_image, r.rgb_image, extras["normal"], extras["confidence"]], [wz, wc, wo, wf])
        assert pc._dcount == dcount, "the backward resolved a device-side count"
        view2 = p.detach().clone().requires_grad_(True)
        n_true = int(pc._count_of(0)[1].item())   # (a read of the device count for the test; the map keeps it)
        assert int(extras["index"].max()) < n_true < bufs[0].shape[0]
        exact = [t.detach()[:n_true].clone().requires_grad_(True) for t in bufs]
        r2 = ops.render_map(*exact, view2[0], frames.intrinsics[0, 0], H, W, radius=1, differentiable=True)
        assert torch.equal(r2.index, extras["index"][0])
        torch.autograd.backward([r2.depth, r2.color, r2.normal, r2.confidence], [wz[0], wc[0], wo[0], wf[0]])
        for a, b in zip(leaves, exact):
            assert torch.equal(a.grad[:n_true], b.grad) and not bool(a.grad[n_true:].any())
            assert bool(torch.isfinite(a.grad).all())
        assert torch.equal(view.grad, view2.grad) and bool(view.grad.any())
        for k, t in zip(("points", "normals", "colors", "features"), bufs):
            pc._buf[k][0] = t
        seen += 1
    assert seen == L - 2


def test_render_loss(gs):
    from gradslam_amd.metrics import depth_residual, render_loss
    c = rc.build("loss6")
    rc.claims(c)
    s, m = rc.scene("small")
    pc, _ = gs.slam.PointFusion(odom="gt", device="cuda")(_frames(gs, s))
    n = len(m)
    bufs = [pc._buf[k][0] for k in ("points", "normals", "colors", "features")]
    stats = depth_residual(pc, _frames(gs, s))
    bufs[0].requires_grad_(True)
    poses = T(s["poses"][None]).cuda().requires_grad_(True)
    frames = _frames(gs, s, poses=poses)
    loss = render_loss(pc, frames)
    assert tuple(loss.shape) == (1, 6) and loss.dtype == torch.float32 and loss.requires_grad and loss.is_cuda
    for f in range(6):
        want = 0.5 * float(stats["rmse"][0, f]) ** 2
        got = float(loss.detach()[0, f])
        print("frame %d: loss %.9g, rmse^2 / 2 %.9g" % (f, got, want))
        # the float64-sum tolerance of tests/test_hip_render.py (1e-9) plus the one rounding of the result to float32
        assert abs(got - want) <= (1e-9 + 2.0 ** -24) * want, (f, got, want)
    loss.sum().backward()
    ref = rc.reference(c)
    gap = dict(zip(rc.OUTPUTS, rc.GAP["loss6"]))
    for name, g, r in (("poses_bar", host(poses.grad[0]), ref[4]), ("points_bar", host(bufs[0].grad)[:n], ref[0])):
        err, bound = bc.rel_err(g, r), bc.kernel_bound(gap[name])
        print("loss6 %s err %.2e bound %.2e" % (name, err, bound))
        assert err <= bound, (name, err, bound)
    assert not host(poses.grad)[0, :, 3].any() and not host(bufs[0].grad)[n:].any()
    # colour term: the value is the masked mean of the squared colour difference, by hand in float64
    lc = render_loss(pc, _frames(gs, s), depth_weight=0.0, color_weight=2.0)
    for f in (0, 3):
        r = rr.render(c.points, c.normals, c.colors, c.ccounts, c.poses[f], c.K, c.H, c.W)
        both = c.both[f]
        d = (r.color.astype(np.float64) - s["colors"][f].astype(np.float64))[both]
        want = 2.0 * 0.5 * (d * d).sum() / both.sum()
        assert abs(float(lc.detach()[0, f]) - want) <= (1e-9 + 2.0 ** -24) * want, (f, float(lc.detach()[0, f]), want)
    # a frame without a pixel valid in both: 0, and a zero gradient, never NaN
    depths = s["depths"].copy()
    depths[2] = 0.0
    poses2 = T(s["poses"][None]).cuda().requires_grad_(True)
    bufs[0].grad = None
    l2 = render_loss(pc, _frames(gs, s, poses=poses2, depths=depths), color_weight=0.5)
    assert float(l2.detach()[0, 2]) == 0.0 and bool(torch.isfinite(l2).all()) and float(l2.detach()[0, 1]) > 0
    l2.sum().backward()
    assert bool(torch.isfinite(poses2.grad).all()) and not bool(poses2.grad[0, 2].any()) and bool(poses2.grad[0, 1].any())
    assert bool(torch.isfinite(bufs[0].grad).all())
