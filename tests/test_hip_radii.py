"""GPU tests of surfel radii: gs_surfel_radius_f32, the model view with radii forward and backward
(gs_render_map_radii_dc_f32, gs_render_map_radii_backward_dc_f32 -> ops.render_map* -> Pointclouds.render), the
SurfelRadii layer through PointFusion and the projective ICP against a view with radii.

References: tests/radii_ref.py (the sample radius, the splat size, the oracle frame loop with the layer rule),
tests/render_radii_ref.py (the view) and the float64 adjoint of tests/render_grad_ref.py on the cases of
tests/render_radii_backward_cases.py.  Images and maps are compared for equal values with the suite's convention (+0 and
-0 compare equal; depth, index, radii and weights by their bits); the backward within backward_cases.kernel_bound(gap)
of the committed CPU gap.  No bound comes from a kernel's output."""
import functools
import warnings

import numpy as np
import pytest
import torch

from gradslam_amd.datasets.synthetic import make_sequence
from tests import backward_cases as bc
from tests import radii_ref
from tests import render_radii_backward_cases as cases
from tests import render_radii_ref as rrr
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

T = torch.from_numpy
FIELDS = ("depth", "color", "normal", "confidence", "index")
NAMES = ("points_bar", "normals_bar", "colors_bar", "ccounts_bar", "poses_bar")


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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


def same_view(got, v, want, what):
    """view v of a RenderedViews (L, ...) against a render_ref.Rendered"""
    for k in FIELDS:
        a, b = host(getattr(got, k)[v]), getattr(want, k)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), "%s %s: %d of %d differ" % (what, k, (a != b).sum(), a.size)
    assert same_bits(host(got.depth[v]), want.depth) and same_bits(host(got.index[v]), want.index), what


class Spy:
    """counts the calls of exports of the loaded library (the calls go through)"""

    def __init__(self, monkeypatch, *names):
        from gradslam_amd import _C
        self.calls = {n: 0 for n in names}
        lib = _C.lib()
        for n in names:
            monkeypatch.setattr(lib, n, self._wrap(n, getattr(lib, n)))

    def _wrap(self, name, fn):
        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


# ------------------------------------------------------------------------------------------ 1. the sample radius
@pytest.mark.parametrize("H,W", [(37, 53), (60, 80)])
def test_sample_radius_equals_the_restatement(ops, H, W):
    B, L = 3, 4
    seqs = [make_sequence(L, H, W, seed=70 + b) for b in range(B)]
    depth = np.stack([s["depths"][..., 0] for s in seqs])                      # (B, L, H, W), holes without depth
    K = np.stack([s["intrinsics"][0] for s in seqs]).astype(np.float32)
    K[1, 1, 1] *= 1.25                                                         # fx != fy somewhere
    rng = np.random.default_rng(5)
    normal = rng.standard_normal((B, L, H, W, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    normal[:, :, 3, 4] = 0.0                   # no normal
    normal[:, :, 5, 6] = (1.0, 0.0, 0.0)       # n_z = 0
    normal[:, :, 7, 8] = (0.6, 0.8, -0.0)      # n_z = -0
    normal[:, :, 9, 10, 1] = np.nan
    normal[:, :, 11, 12, 0] = np.inf
    normal[:, :, 13, 14] = (0.0, 0.0, 1e-30)   # r0 / c overflows: the cap
    depth[:, :, 15, 16] = -1.0
    assert (depth == 0).any() and (depth[:, :, 3, 4] > 0).any() and (depth[:, :, 5, 6] > 0).any()
    want = [[radii_ref.surfel_radius(depth[b, s], normal[b, s], K[b]) for s in range(L)] for b in range(B)]
    assert any(w[0][5, 6] > 0 and w[0][13, 14] > 0 and not w[1][3, 4] and not w[1][9, 10] for row in want for w in row)
    D, N, Kd = dev(depth), dev(normal), dev(K)
    # the whole stack, a non-contiguous slice of it, one image
    rho, valid = ops.surfel_radius(D, N, Kd.unsqueeze(1).expand(B, L, 4, 4))
    assert rho.shape == (B, L, H, W) and rho.dtype == torch.float32 and valid.dtype == torch.bool
    for b in range(B):
        for s in range(L):
            assert same_bits(host(rho[b, s]), want[b][s][0]) and np.array_equal(host(valid[b, s]), want[b][s][1]), (b, s)
    sl_d, sl_n = D[:, 2], N[:, 2]
    assert not sl_d.is_contiguous() and not sl_n.is_contiguous()
    rho, valid = ops.surfel_radius(sl_d, sl_n, Kd)
    for b in range(B):
        assert same_bits(host(rho[b]), want[b][2][0]) and np.array_equal(host(valid[b]), want[b][2][1]), b
    rho, valid = ops.surfel_radius(D[1, 3], N[1, 3], Kd[1])
    assert rho.shape == (H, W) and same_bits(host(rho), want[1][3][0]) and np.array_equal(host(valid), want[1][3][1])
    # channels of a wider normal stack: the images are not contiguous, the call copies them
    wide = torch.zeros((B, H, W, 5), device="cuda")
    wide[..., :3] = N[:, 0]
    rho, _ = ops.surfel_radius(D[:, 0], wide[..., :3], Kd)
    for b in range(B):
        assert same_bits(host(rho[b]), want[b][0][0]), b


# ------------------------------------------------------------------------------------------ 2. the forward
def hip_render(ops, c, **more):
    n_dev = None if c.n == len(c.points) else torch.tensor([c.n], dtype=torch.int64, device="cuda")
    return ops.render_map(dev(c.points), dev(c.normals), dev(c.colors), dev(c.ccounts), dev(c.poses), dev(c.K), c.H, c.W,
                          n_dev=n_dev, radii=dev(c.radii), max_radius=c.max_radius, **c.kw, **more)


@pytest.mark.parametrize("name", ["cap0", "filters", "layer_near", "odd_count", "span_cap3", "span_cap8"])
def test_forward_equals_the_restatement(ops, name):
    """L = 1, 2, 3, 4 and 5 views; max_radius 0, 3 and 8; every r of 0 ... max_radius, rows clipped at each border, ties,
    radii that are 0, negative, NaN and inf (span_*), both filters (filters), a device-side count below the bound
    (odd_count): each asserted on the restatement by cases.claims"""
    c = cases.build(name)
    cases.claims(c)
    got = hip_render(ops, c)
    for v in range(len(c.poses)):
        same_view(got, v, c.images[v], "%s view %d" % (name, v))
    again = hip_render(ops, c)
    for k in FIELDS:
        assert torch.equal(getattr(got, k), getattr(again, k)), (name, k)


@pytest.mark.parametrize("B", [3, 9])
def test_forward_of_a_batch(ops, B):
    """B = 3 and 9 sequences (more than the 8 of one launch) of different sizes, 5 views each in a different order, one
    with a device-side count; sequence b is exactly the call of its own"""
    c = cases.build("span_cap8")
    sizes = [len(c.points), 4000, 1, 2500, 100, 4576 - 37, 3000, 777, 2000][:B]
    maps, radii, refs, poses = [], [], [], []
    for b, n in enumerate(sizes):
        counted = b == 2 or b == 5          # (the bound stays the buffer's rows)
        rows = len(c.points) if counted else n
        n_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if counted else None
        maps.append(ops.MapRows(dev(c.points[:rows]), dev(c.normals[:rows]), dev(c.colors[:rows]), dev(c.ccounts[:rows]),
                                None, n_dev))
        radii.append(dev(c.radii[:rows]))
        P = np.roll(c.poses, b, axis=0)
        poses.append(P)
        refs.append([rrr.render(c.points[:n], c.normals[:n], c.colors[:n], c.ccounts[:n], c.radii[:n], P[v], c.K, c.H,
                                c.W, 8)[0] for v in range(5)])
    got = ops.render_map_batch(maps, dev(np.stack(poses)), dev(np.stack([c.K] * B)), c.H, c.W, radii=radii, max_radius=8)
    assert got.depth.shape == (B, 5, c.H, c.W, 1) and got.index.shape == (B, 5, c.H, c.W)
    for b in range(B):
        one = type(got)(*[t[b] for t in got])
        for v in range(5):
            same_view(one, v, refs[b][v], "sequence %d view %d" % (b, v))


# ------------------------------------------------------------------------------------------ 3. against the old entry
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_constant_r_gives_the_bits_of_radius_k(ops, monkeypatch, k):
    s, m, lay = cases.scene("wave")
    K = s["intrinsics"][0].astype(np.float32)
    H, W = s["depths"].shape[1:3]
    spy = Spy(monkeypatch, "gs_render_map_dc_f32", "gs_render_map_radii_dc_f32")
    arrays = [dev(a) for a in (m.points, m.normals, m.colors, m.ccounts)]
    for view in ("0", "o1", "z+0.4"):
        pose = cases.view_pose(s, view)
        _, key = rr.row_keys(m.points, m.normals, m.ccounts, pose, K, H, W)
        z = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        with np.errstate(all="ignore"):
            radii = ((np.float32(k + 0.5) * z) / radii_ref.fbar_of(K)).astype(np.float32)
        pix, _, r = rrr.row_splats(m.points, m.normals, m.ccounts, radii, pose, K, H, W, max_radius=3)
        assert (pix >= 0).sum() > 500 and (r[pix >= 0] == k).all(), "the reference reports r = %d for every row" % k
        before = dict(spy.calls)
        old = ops.render_map(*arrays, dev(pose), dev(K), H, W, radius=k)
        assert spy.calls == dict(before, gs_render_map_dc_f32=before["gs_render_map_dc_f32"] + 1), \
            "radii=None launches the old entry"
        new = ops.render_map(*arrays, dev(pose), dev(K), H, W, radii=dev(radii), max_radius=3)
        assert spy.calls["gs_render_map_radii_dc_f32"] == before["gs_render_map_radii_dc_f32"] + 1
        assert spy.calls["gs_render_map_dc_f32"] == before["gs_render_map_dc_f32"] + 1
        for f in FIELDS:
            assert same_bits(host(getattr(old, f)), host(getattr(new, f))), (k, view, f)
        assert (host(new.index) >= 0).mean() > 0.1


def test_the_old_backward_entry_serves_calls_without_radii(ops, monkeypatch):
    c = cases.build("cap0")
    spy = Spy(monkeypatch, "gs_render_map_backward_dc_f32", "gs_render_map_radii_backward_dc_f32")
    leaves = [dev(a).requires_grad_(True) for a in (c.points, c.normals, c.colors, c.ccounts)]
    r = ops.render_map(*leaves, dev(c.poses), dev(c.K), c.H, c.W, differentiable=True)
    r.depth.sum().backward()
    assert spy.calls == {"gs_render_map_backward_dc_f32": 1, "gs_render_map_radii_backward_dc_f32": 0}
    r = ops.render_map(*leaves, dev(c.poses), dev(c.K), c.H, c.W, differentiable=True, radii=dev(c.radii), max_radius=2)
    r.depth.sum().backward()
    assert spy.calls == {"gs_render_map_backward_dc_f32": 1, "gs_render_map_radii_backward_dc_f32": 1}


# ------------------------------------------------------------------------------------------ 4. the backward
def upstream(c):
    out = []
    for a, tail in ((c.zb, (1,)), (c.cb, (3,)), (c.ob, (3,)), (c.fb, (1,))):
        out.append(None if a is None else dev(a.reshape(c.index.shape + tail)))
    return out


def hip_grads(ops, c):
    leaves = [dev(a).requires_grad_(True) for a in (c.points, c.normals, c.colors, c.ccounts)]
    P = dev(c.poses).requires_grad_(True)
    K = dev(c.K).requires_grad_(True)
    rho = dev(c.radii).requires_grad_(True)
    n_dev = None if c.n == len(c.points) else torch.tensor([c.n], dtype=torch.int64, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = ops.render_map(*leaves, P, K, c.H, c.W, n_dev=n_dev, differentiable=True, radii=rho,
                           max_radius=c.max_radius, **c.kw)
    assert np.array_equal(host(r.index), c.index), "the HIP winners are the restated ones"
    assert same_bits(host(r.depth)[..., 0], c.depth)
    pairs = [(img, up) for img, up in zip((r.depth, r.color, r.normal, r.confidence), upstream(c)) if up is not None]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
    assert K.grad is None and rho.grad is None, "K and the radii are constants of the gradient"
    return [None if t.grad is None else host(t.grad) for t in leaves] + [host(P.grad)]


def within(c, got):
    ref = cases.reference(c)
    gap = dict(zip(cases.OUTPUTS, cases.GAP[c.name]))
    n = c.n
    for name, g, r in zip(NAMES, got, ref):
        assert g is not None and g.dtype == np.float32 and np.isfinite(g).all(), (c.name, name)
        if name != "poses_bar":
            g = g.reshape(g.shape[0], -1)
            r = r.reshape(r.shape[0], -1)
            assert g.shape[0] == len(c.points) and not g[n:].any(), "%s: %s is not zero beyond the count" % (c.name, name)
            g = g[:n]
        assert g.shape == r.shape, (c.name, name, g.shape, r.shape)
        if not np.abs(r).max() > 0:
            assert not g.any(), "%s: %s must be exactly zero" % (c.name, name)
            continue
        bound = bc.kernel_bound(gap[name]) if gap.get(name) is not None else bc.kernel_bound(0.0)
        err = bc.rel_err(g, r)
        print("%-12s %-11s err %.2e bound %.2e" % (c.name, name, err, bound))
        assert err <= bound, (c.name, name, err, bound)
    won = np.zeros(n, bool)
    won[c.index[c.index >= 0]] = True
    for name, g in zip(NAMES[:4], got[:4]):
        assert not g[:n][~won].any(), "%s: %s of a row that wins nothing" % (c.name, name)
    assert not got[4][:, 3].any(), "%s: bottom row of poses_bar" % c.name


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_backward_equals_float64_adjoint(ops, name):
    c = cases.build(name)
    cases.claims(c)
    got = hip_grads(ops, c)
    within(c, got)
    again = hip_grads(ops, c)
    for n_, a, b in zip(NAMES, got, again):
        assert same_bits(a, b), "%s: two identical calls differ in %s" % (name, n_)


def test_outputs_that_are_not_asked_for_are_skipped(ops):
    c = cases.build("layer_near")
    ref = cases.reference(c)
    maps = [(dev(c.points), dev(c.normals), None, None)]
    args = (dev(c.poses[None]), dev(c.K[None]), dev(c.index[None]), [u if u is None else u[None] for u in upstream(c)],
            c.H, c.W)
    kw = dict(radii=[dev(c.radii)], max_radius=c.max_radius)
    full, T_full = ops.render_map_backward_batch(maps, *args, **kw)
    rows, T_bar = ops.render_map_backward_batch(maps, *args, want=(True, False, False, True, False), **kw)
    assert T_bar is None and rows[0][1] is None and rows[0][2] is None
    assert torch.equal(rows[0][0], full[0][0]) and torch.equal(rows[0][3], full[0][3])
    assert bc.rel_err(host(rows[0][0]), ref[0]) <= bc.kernel_bound(cases.GAP[c.name][0])
    rows, T_bar = ops.render_map_backward_batch(maps, *args, want=(False, False, False, False, True), **kw)
    assert all(t is None for t in rows[0]) and torch.equal(T_bar, T_full)
    # a loss on one image through autograd: the other images reach the kernel as NULL
    leaves = [dev(a).requires_grad_(i == 2) for i, a in enumerate((c.points, c.normals, c.colors, c.ccounts))]
    r = ops.render_map(*leaves, dev(c.poses), dev(c.K), c.H, c.W, differentiable=True, radii=dev(c.radii),
                       max_radius=c.max_radius)
    (r.color * dev(c.cb)).sum().backward()
    assert leaves[0].grad is None and leaves[1].grad is None and leaves[3].grad is None
    assert bc.rel_err(host(leaves[2].grad), ref[2]) <= bc.kernel_bound(0.0)


# ------------------------------------------------------------------------------------------ 5. the layer
LB, LL, LH, LW = 2, 5, 37, 53
SCHEDULES = dict(carve_margin=0.05, carve_window=1, voxel_size=0.03, prune_min_confidence=3e-7, prune_min_age=0,
                 prune_every=2)      # (at this frame size the sample confidences sit at the 1e-7 clamp and a little above)


@functools.lru_cache(maxsize=None)
def layer_sequences():
    """two sequences of 5 frames; a block of the first two frames is measured 0.4 m nearer, so that the carve of the
    later frames has something to remove"""
    seqs = [make_sequence(LL, LH, LW, seed=60 + b) for b in range(LB)]
    for s in seqs:
        d = s["depths"].copy()
        blk = d[:2, 10:20, 15:30]
        blk[blk > 0] -= 0.4
        s["depths"] = d
    return seqs


def layer_frames(gs):
    seqs = layer_sequences()
    st = lambda k: T(np.stack([s[k] for s in seqs])).cuda()      # noqa: E731
    return gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), st("poses"))


def snapshot(pc):
    lay = pc.map_features
    n = [int(t.shape[0]) for t in pc.points_list]
    assert [int(t.shape[0]) for t in lay.radii_list] == n == [int(t.shape[0]) for t in lay.weights_list], "row-aligned"
    return [dict(points=host(pc.points_list[b]), normals=host(pc.normals_list[b]), colors=host(pc.colors_list[b]),
                 ccounts=host(pc.features_list[b]), radius=host(lay.radii_list[b]), weight=host(lay.weights_list[b]))
            for b in range(len(n))]


def oracle_layers(poses, schedules):
    """the oracle frame loop with the restated layer rule under the poses the driver recovered"""
    out = []
    kw = {}
    if schedules:
        kw = dict(carve=dict(margin=SCHEDULES["carve_margin"], window=SCHEDULES["carve_window"]),
                  voxel_size=SCHEDULES["voxel_size"],
                  prune=dict(min_confidence=SCHEDULES["prune_min_confidence"], every=SCHEDULES["prune_every"]))
    for b, s in enumerate(layer_sequences()):
        sizes = []
        m, lay = radii_ref.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], poses[b], **kw,
                                        per_frame=lambda f, m_, l_: sizes.append(len(m_)))
        out.append((m, lay, sizes))
    return out


def same_maps(snap, want, what):
    for b, (m, lay, _) in enumerate(want):
        g = snap[b]
        assert len(g["points"]) == len(m), (what, b, len(g["points"]), len(m))
        for k in ("points", "normals", "colors", "ccounts"):
            assert np.array_equal(g[k].reshape(len(m), -1), getattr(m, k).reshape(len(m), -1)), (what, b, k)
        assert same_bits(g["radius"], lay.radius), (what, b, "radius", int((g["radius"] != lay.radius).sum()))
        assert same_bits(g["weight"], lay.weight), (what, b, "weight")


@pytest.mark.parametrize("schedules", [False, True])
@pytest.mark.parametrize("how", ["step_fast", "step_generic", "forward"])
def test_the_layer_equals_the_oracle_loop_with_the_layer_rule(gs, how, schedules):
    """PointFusion(surfel_radii=True) through step on the one-call path (gradicp), through step on the generic path
    (ground-truth odometry) and through forward, without and with the carve, thinning and pruning schedules"""
    frames = layer_frames(gs)
    odom = "gt" if how == "step_generic" else "gradicp"
    slam = gs.slam.PointFusion(odom=odom, dsratio=2, device="cuda", surfel_radii=True, **(SCHEDULES if schedules else {}))
    if how == "forward":
        pc, poses = slam.forward(frames)
    else:
        pc = gs.Pointclouds(device="cuda").attach_features(gs.SurfelRadii())
        prev, rec = None, []
        for s in range(LL):
            live = frames[:, s]         # (its ground-truth pose is read by odom="gt" and by the first step only)
            pc, p = slam.step(pc, live, prev, inplace=True)
            prev = live if odom != "gt" else None
            rec.append(p[:, 0])
        poses = torch.stack(rec, 1)
        assert (getattr(slam, "_step_plan", None) is not None) == (how == "step_fast"), "the path the test is about"
    assert isinstance(pc.map_features, gs.SurfelRadii)
    want = oracle_layers(host(poses), schedules)
    if schedules:
        plain = oracle_layers(host(poses), False)
        assert all(len(w[0]) < len(p[0]) for w, p in zip(want, plain)) and all(len(w[0]) > 500 for w in want), \
            "the schedules remove rows and leave a map"
    same_maps(snapshot(pc), want, (how, schedules))
    for m, lay, _ in want:
        assert (lay.radius > 0).mean() > 0.9
    # the view with the layer's radii is the restated one
    K = frames.intrinsics
    view = pc.render(K, poses[:, -1:].contiguous(), LH, LW, radii="layer", return_extras=True)
    for b, (m, lay, _) in enumerate(want):
        ref = rrr.render(m.points, m.normals, m.colors, m.ccounts, lay.radius, host(poses)[b, -1],
                         layer_sequences()[b]["intrinsics"][0], LH, LW, 3)[0]
        assert same_bits(host(view[0].depth_image[b, 0]), ref.depth) and same_bits(host(view[1]["index"][b, 0]), ref.index)


def test_depth_filter_reaches_the_layer(gs):
    """the layer samples the frame the map update saw: with depth_filter the radii differ from the unfiltered run's, and
    the weight stays the confidence count where every sample had a normal"""
    frames = layer_frames(gs)
    runs = []
    for kw in ({}, dict(depth_filter=dict(radius=1))):
        pc, _ = gs.slam.PointFusion(odom="gt", device="cuda", surfel_radii=True, **kw).forward(frames)
        runs.append(snapshot(pc))
    for b in range(LB):
        a, f = runs[0][b], runs[1][b]
        assert (f["weight"] <= f["ccounts"].reshape(-1)).all()
        assert (f["weight"].view(np.uint32) == f["ccounts"].reshape(-1).view(np.uint32)).mean() > 0.8
        n = min(len(a["radius"]), len(f["radius"]))
        assert (a["radius"][:n] != f["radius"][:n]).mean() > 0.5


# ------------------------------------------------------------------------------------------ 6. the odometry
def test_projicp_with_surfel_radii_equals_the_hand_written_loop(gs, ops, monkeypatch):
    frames = layer_frames(gs)
    spy = Spy(monkeypatch, "gs_render_map_dc_f32", "gs_render_map_radii_dc_f32")

    def run(**kw):
        slam = gs.slam.PointFusion(odom="projicp", dsratio=2, device="cuda", surfel_radii=True, **kw)
        pc = gs.Pointclouds(device="cuda").attach_features(gs.SurfelRadii())
        prev, rec = None, []
        for s in range(LL):
            live = frames[:, s]         # (the first step reads its pose; later steps overwrite theirs)
            pc, p = slam.step(pc, live, prev, inplace=True)
            prev = live
            rec.append(p[:, 0])
        return pc, torch.stack(rec, 1)

    pc, poses = run(odom_surfel_radii=True)
    assert spy.calls == {"gs_render_map_dc_f32": 0, "gs_render_map_radii_dc_f32": LL - 1}
    # by hand: the view with the layer's radii, the plain solve on its index image, the map update under that pose
    upd = gs.slam.PointFusion(odom="gt", device="cuda", surfel_radii=True)
    pc2 = gs.Pointclouds(device="cuda").attach_features(gs.SurfelRadii())
    K = frames.intrinsics[:, 0].contiguous()
    prev, rec = None, []
    for s in range(LL):
        live = frames[:, s]
        if s > 0:
            radii = pc2.map_features.radii_list
            maps = pc2._map_rows(("points", "normals"))
            view = ops.render_map_batch([m._replace(normals=None) for m in maps], prev.view(LB, 1, 4, 4), K, LH, LW,
                                        radii=radii, max_radius=3)
            fr = live.to_channels_last()
            pose = ops.projective_icp_batch(fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K,
                                            view.index[:, 0], prev, maps, prev, stride=2, numiters=20, damp=1e-8,
                                            dist_thresh=0.1, angle_thresh=30)
            live.poses = pose.view(LB, 1, 4, 4)
        pc2, p = upd.step(pc2, live, None, inplace=True)
        prev = p[:, 0].contiguous()
        rec.append(prev)
    hand = torch.stack(rec, 1)
    assert same_bits(host(poses), host(hand)), "the pose bits of the hand-written loop"
    a, b = snapshot(pc), snapshot(pc2)
    for x, y in zip(a, b):
        for k in x:
            assert same_bits(x[k], y[k]), k
    # the default: the old entry, and the poses and the map of a run without the layer
    before = dict(spy.calls)
    pc3, poses3 = run()
    assert spy.calls == dict(before, gs_render_map_dc_f32=before["gs_render_map_dc_f32"] + LL - 1)
    slam = gs.slam.PointFusion(odom="projicp", dsratio=2, device="cuda")
    pc4, prev, rec = gs.Pointclouds(device="cuda"), None, []
    for s in range(LL):
        live = frames[:, s]
        pc4, p = slam.step(pc4, live, prev, inplace=True)
        prev = live
        rec.append(p[:, 0])
    assert same_bits(host(poses3), host(torch.stack(rec, 1))), "without odom_surfel_radii: today's poses"
    for b in range(LB):
        assert torch.equal(pc3.points_list[b], pc4.points_list[b]) and torch.equal(pc3.features_list[b], pc4.features_list[b])


COMBOS = {
    "color": dict(color_weight=0.05 / 255),
    "huber_k": dict(huber_k=1.345, huber_delta=0.002),
    "pixel_weights": dict(odom_pixel_weights="axial"),
    "outlier_mask": dict(odom_outlier_mask=dict(refine_iters=3)),
    "outliers_not_fused": dict(odom_outlier_mask=dict(refine_iters=3), fuse_outliers=False),
    "taped": dict(odom_differentiable=True),
}


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_surfel_radii_change_the_view_and_nothing_else_of_the_solve(gs, ops, monkeypatch, combo):
    """odom_surfel_radii with the colour term, a Huber scale, pixel weights, the outlier mask (fused and not fused) and on
    the autograd tape: the poses, the map and the layer of the driver are, bit for bit, those of the same driver WITHOUT
    the switch whose one render call per localisation is handed the layer's radii from outside"""
    frames = layer_frames(gs)
    kw = dict(COMBOS[combo])
    if kw.get("odom_pixel_weights") == "axial":
        kw["odom_pixel_weights"] = gs.odometry.axial_noise_weights
    state = {}

    def run(**more):
        slam = gs.slam.PointFusion(odom="projicp", dsratio=2, device="cuda", surfel_radii=True, **kw, **more)
        pc = state["pc"] = gs.Pointclouds(device="cuda").attach_features(gs.SurfelRadii())
        prev, rec = None, []
        for s in range(LL):
            live = frames[:, s]
            pc, p = slam.step(pc, live, prev, inplace=True)
            prev = live
            rec.append(p[:, 0].detach())
        return snapshot(pc), host(torch.stack(rec, 1))

    spy = Spy(monkeypatch, "gs_render_map_dc_f32", "gs_render_map_radii_dc_f32")
    snap, poses = run(odom_surfel_radii=True)
    assert spy.calls == {"gs_render_map_dc_f32": 0, "gs_render_map_radii_dc_f32": LL - 1}
    assert np.isfinite(poses).all()
    plain = ops.render_map_batch

    def with_radii(maps, *args, **kwargs):
        assert "radii" not in kwargs
        lay = state["pc"].map_features
        radii = [lay._emb[b][:min(m.n_bound, int(m.points.shape[0])), 0] for b, m in enumerate(maps)]
        return plain(maps, *args, radii=radii, max_radius=3, **kwargs)
    monkeypatch.setattr(ops, "render_map_batch", with_radii)
    snap2, poses2 = run()
    assert spy.calls == {"gs_render_map_dc_f32": 0, "gs_render_map_radii_dc_f32": 2 * (LL - 1)}
    assert same_bits(poses, poses2), combo
    for x, y in zip(snap, snap2):
        for k in x:
            assert same_bits(x[k], y[k]), (combo, k)
        assert (x["radius"] > 0).mean() > 0.5 and len(x["radius"]) > 500, "a map with radii"
