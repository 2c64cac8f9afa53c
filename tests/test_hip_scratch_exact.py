"""GPU table of every scratch user: each entry runs on scratch buffers of EXACTLY the size its sizer reports, between
guard bands, poisoned with three different bytes (tests/scratch_guard.py).

Per row, four runs: (a) a plain call, then the same call inside `exact_scratch` with fills 0x00, 0xFF (NaN / -1) and 0x7F
(a large finite float / a large positive int).  Per guarded run:

* both guards of every buffer are intact after the stream has drained: nothing wrote before or behind its scratch;
* the logged requests are the row's: the names, and per name the value the test computes from the sizer export for the
  arguments the row states (a row cannot pass by asking for no scratch, or for a generous one);
* the outputs equal run (a) bit for bit wherever the entry's own test asserts equal bits or run-to-run reproducibility;
  where that test lets two runs of atomic float64 sums differ (the map gradients of the projective ICP backward in its
  atomic mode, the grid-search ICP backward without GRADSLAM_HIP_DETERMINISTIC_BACKWARD) the bound is its bound,
  backward_cases.kernel_bound(0.0) on backward_cases.rel_err.  No other tolerance exists here.

A guard that was written on is a short sizer, a carve that disagrees with it, or wrong sizer arguments of the caller; an
output that follows the fill is a read before write.  The only accepted dependence on earlier scratch contents is the
documented hand-over from a localisation to the stats exporters, exercised inside ONE context.

What guards cannot see: READS past the end of a scratch (the list engines' unconditional row loads are one case).  They
land in the guard and leave it as it was; only the comparison of the outputs under three fills covers them.

Inputs come from the case builders and restatements of the entries' own tests; no reference is written here.  ROWS is
also what tests/test_scratch_guard_cpu.py holds complete: every workspace name of ops.py / slam/_fastpath.py and every
*_scratch_bytes export must be named by a row."""
import collections
import functools

import numpy as np
import pytest
import torch

from gradslam_amd import _C
from tests import backward_cases as bc
from tests import scratch_guard as sg
from tests.test_hip_picp_weighted import GEO, JOINT

gpu = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x7F)
SUM_BOUND = bc.kernel_bound(0.0)     # two runs of the same float64 atomic sums, rounded once (test_hip_picp_backward.MAP_BOUND)
SIGMA, DIST_TH, DOT_TH = 0.6, 0.05, 0.9
FRAMES = {"24x40": (24, 40), "37x53": (37, 53)}     # 960 px: under one 1024 tile; 1961 px: two tiles
MAP_ROWS = (300, 1024, 1025)

Row = collections.namedtuple("Row", ["id", "names", "sizers", "fn"])
ROWS = []


def row(rid, names, sizers):
    """registers fn(ctx) -> [(label, value, "bits" | "sums")]: `names` the workspace names it must log (a %d stands for
    the sequence), `sizers` the exports its expected sizes must come from"""
    def deco(fn):
        ROWS.append(Row(rid, tuple(names), tuple(sizers), fn))
        return fn
    return deco


def table_names():
    return {n for r in ROWS for n in r.names}


def table_sizers():
    return {s for r in ROWS for s in r.sizers}


class Ctx(object):
    """what a row sees: ops, the library, `expect(name, sizer, *args)` to state a request, `buffer(name, nbytes)` for a
    buffer the caller hands to an entry itself (a tape), guarded like the scratch when the run is a guarded one"""

    def __init__(self, ops, monkeypatch, log=None):
        self.ops, self.L, self.mp, self.log = ops, _C.lib(), monkeypatch, log
        self.expected, self.used = [], set()

    def size(self, sizer, *args):
        self.used.add(sizer)
        return int(getattr(self.L, sizer)(*[int(a) for a in args]))

    def expect(self, name, sizer, *args):
        self.expected.append((name, self.size(sizer, *args)))

    def buffer(self, name, nbytes):
        self.expected.append((name, int(nbytes)))
        if self.log is None:
            return torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")[:int(nbytes)]
        return sg.guarded_buffer(self.log, name, nbytes, "cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def flat(x, label="out"):
    """every tensor / array / number inside nested tuples, lists and namedtuples, labelled by its path"""
    if x is None:
        return [(label, None)]
    if torch.is_tensor(x):
        return [(label, x.detach().cpu().numpy().copy())]
    if isinstance(x, np.ndarray):
        return [(label, x.copy())]
    if isinstance(x, dict):
        return [p for k in sorted(x) for p in flat(x[k], "%s.%s" % (label, k))]
    if isinstance(x, (tuple, list)):
        return [p for i, v in enumerate(x) for p in flat(v, "%s[%d]" % (label, i))]
    return [(label, np.asarray(x))]


def bits_of(x, label="out"):
    return [(lb, v, "bits") for lb, v in flat(x, label)]


def sums_of(x, label="out"):
    return [(lb, v, "sums") for lb, v in flat(x, label)]


def pattern_of(name):
    """localize1 -> localize%d where the table knows that pattern"""
    stem = name.rstrip("0123456789")
    return stem + "%d" if stem != name and stem + "%d" in table_names() else name


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


def compare(rid, fill, base, got):
    assert [b[0] for b in base] == [g[0] for g in got], (rid, "the outputs of two runs have different shapes")
    for (label, a, kind), (_, b, _) in zip(base, got):
        what = "%s %s with fill 0x%02X" % (rid, label, fill)
        if a is None or b is None:
            assert a is None and b is None, what
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, what
        if kind == "bits":
            assert a.tobytes() == b.tobytes(), what + ": the result depends on what the scratch held (read before write)"
        else:
            err = bc.rel_err(b, a)
            print("%-60s err %.2e bound %.2e" % (what, err, SUM_BOUND))
            assert np.isfinite(b).all() and err <= SUM_BOUND, (what, err, SUM_BOUND)


def run_row(r, ops, monkeypatch):
    ctx = Ctx(ops, monkeypatch)
    base = r.fn(ctx)
    torch.cuda.synchronize()
    for fill in FILLS:
        with sg.exact_scratch(monkeypatch, fill) as log:
            ctx = Ctx(ops, monkeypatch, log)
            got = r.fn(ctx)
            torch.cuda.synchronize()
            ok, hits = sg.intact(log)
            asked = sg.requests(log)
        assert ok, (r.id, "fill 0x%02X" % fill, "written outside an exact scratch: short sizer, carve or sizer arguments", hits)
        assert sorted(asked) == sorted(ctx.expected), (r.id, "requests", sorted(asked), "expected", sorted(ctx.expected))
        # (a "tape*" buffer is the caller's own, handed to the entry next to the scratch: no workspace name, so it is held by
        # the equality above alone)
        assert {pattern_of(n) for n, _ in asked if not n.startswith("tape")} == set(r.names), (r.id, asked, r.names)
        assert ctx.used == set(r.sizers), (r.id, ctx.used, r.sizers)
        compare(r.id, fill, base, got)


# =========================================================================================== compaction scratch ("scratch")
_SCENES = {}


def cscene(ops, size, n):
    """one frame and a map of n rows on the device, with the tables the table-level entries take; built once by run (a),
    outside any guarded context, and left alone"""
    if (size, n) not in _SCENES:
        from tests import test_hip_update_fewer_gathers as ufg
        H, W = FRAMES[size]
        s = ufg.Rows(ufg.make_frame(H, W, 11)).fill(n).seq()
        assert s["P"].shape[0] == n
        d = {k: dev(s[k]) for k in s}
        d.update(H=H, W=W, n=n)
        d["pix"] = ops.project_map(d["P"], d["pose"], d["K"], H, W)
        d["act"] = ops.active_table(d["pix"], W)
        mask = ops.similar_rows(d["act"], d["P"], d["N"], d["gvertex"], d["gnormal"], DIST_TH, DOT_TH)
        d["sim_rows"] = d["act"][mask].contiguous()
        d["best"] = ops.associate(d["pix"], d["P"], d["N"], d["F"], d["gvertex"], d["gnormal"], DIST_TH, DOT_TH)
        d["n_dev"] = torch.tensor([n], dtype=torch.int64, device="cuda")
        assert d["act"].shape[0] > 20 and d["sim_rows"].shape[0] > 5 and int((d["best"] >= 0).sum()) > 5
        torch.cuda.synchronize()
        _SCENES[(size, n)] = d
    return _SCENES[(size, n)]


def store(d, attrs="PNCF"):
    """capacity-backed copy of the map: n + H*W rows, NaN behind the map"""
    out = []
    for k in attrs:
        b = torch.full((d["n"] + d["H"] * d["W"], d[k].shape[1]), float("nan"), dtype=torch.float32, device="cuda")
        b[:d["n"]] = d[k]
        out.append(b)
    return out


def compaction(entry):
    """one row per frame size and map size for `entry(ctx, d) -> outputs`, which states its gs_scratch_bytes arguments"""
    for size in sorted(FRAMES):
        for n in MAP_ROWS:
            def fn(ctx, size=size, n=n):
                return entry(ctx, cscene(ctx.ops, size, n))
            row("%s[%s-%d]" % (entry.__name__, size, n), ["scratch"], ["gs_scratch_bytes"])(fn)
    return entry


@compaction
def downsample_frame(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", 0, d["H"] * d["W"])
    return bits_of(ctx.ops.downsample_frame(d["gvertex"], d["gnormal"], d["rgb"], d["depth"], 4))


@compaction
def active_table(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], 0)
    return bits_of(ctx.ops.active_table(d["pix"], d["W"]))


@compaction
def select_targets_cap(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], 0)
    out = ctx.ops.select_targets(d["pix"], d["W"], 4, d["P"], d["N"], d["C"], cap=160)     # (at most 10 x 14 lattice pixels)
    assert out[0].shape[0] > 5
    return bits_of(out)


@compaction
def downsample_table(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["act"].shape[0], 0)
    return bits_of(ctx.ops.downsample_table(d["act"], 4, d["P"], d["N"], d["C"]))


@compaction
def best_unique_rows(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["sim_rows"].shape[0], d["H"] * d["W"])
    return bits_of(ctx.ops.best_unique_rows(d["sim_rows"], d["P"], d["F"], d["gvertex"]))


@compaction
def associate(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], d["H"] * d["W"])
    return bits_of(ctx.ops.associate(d["pix"], d["P"], d["N"], d["F"], d["gvertex"], d["gnormal"], DIST_TH, DOT_TH,
                                     want_similar=True))


@compaction
def associate_n_dev(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], d["H"] * d["W"])
    return bits_of(ctx.ops.associate(d["pix"], d["P"], d["N"], d["F"], d["gvertex"], d["gnormal"], DIST_TH, DOT_TH,
                                     want_similar=True, n_dev=d["n_dev"]))


@compaction
def best_table(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", 0, d["H"] * d["W"])
    return bits_of(ctx.ops.best_table(d["best"], d["H"], d["W"]))


def _fuse(ctx, d, n_dev):
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], d["H"] * d["W"])
    bufs = store(d)
    cnt = ctx.ops.fuse_append_(*bufs, d["n"], d["best"], d["gvertex"], d["gnormal"], d["rgb"], d["alpha"], d["depth"], True,
                               n_dev=n_dev)
    assert cnt > d["n"]
    return bits_of([cnt] + bufs)


@compaction
def fuse_append_(ctx, d):
    return _fuse(ctx, d, None)


@compaction
def fuse_append_n_dev(ctx, d):
    return _fuse(ctx, d, d["n_dev"])


def _append_valid(ctx, d, n_dev):
    """no direct GPU test of its own: compared with tensor[mask] in raster order, as structures/utils.py uses it"""
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], d["H"] * d["W"])
    bufs = store(d, "PNC")
    cnt = ctx.ops.append_valid_(bufs[0], bufs[1], bufs[2], None, d["n"], d["gvertex"], d["gnormal"], d["rgb"], None,
                                d["depth"], n_dev=n_dev)
    mask = (d["depth"] > 0).reshape(-1)
    assert cnt == d["n"] + int(mask.sum()) and int(mask.sum()) > 100
    for b, k, img in zip(bufs, "PNC", ("gvertex", "gnormal", "rgb")):
        assert torch.equal(b[:d["n"]].view(torch.int32), d[k].view(torch.int32)), "the old rows moved"
        assert torch.equal(b[d["n"]:cnt].view(torch.int32), d[img].reshape(-1, 3)[mask].view(torch.int32)), img
        assert bool(torch.isnan(b[cnt:]).all()), "rows beyond the new count were written"
    return bits_of([cnt] + bufs)


@compaction
def append_valid_(ctx, d):
    return _append_valid(ctx, d, None)


@compaction
def append_valid_n_dev(ctx, d):
    return _append_valid(ctx, d, d["n_dev"])


@compaction
def fuse_append_backward(ctx, d):
    """FuseAppendFunction: the forward and the backward ask for the same gs_scratch_bytes(n, H W): one request"""
    ctx.expect("scratch", "gs_scratch_bytes", d["n"], d["H"] * d["W"])
    leaves = [d[k].clone().requires_grad_(True) for k in ("P", "N", "C", "F", "gvertex", "gnormal", "rgb", "alpha")]
    outs = ctx.ops.FuseAppendFunction.apply(*leaves, d["depth"], d["best"], True)
    torch.autograd.backward(outs, [dev(bc.weights(tuple(o.shape), 50 + i)) for i, o in enumerate(outs)])
    return bits_of([t.grad for t in leaves])


@compaction
def downsample_frame_backward(ctx, d):
    ctx.expect("scratch", "gs_scratch_bytes", 0, d["H"] * d["W"])
    gv = d["gvertex"].clone().requires_grad_(True)
    pts = ctx.ops.DownsampleFramePointsFunction.apply(gv, d["depth"], 4)
    pts.backward(dev(bc.weights(tuple(pts.shape), 60)))
    return bits_of(gv.grad)


# =========================================================================================== knn_grid
def _knn_clouds(ns, nt):
    """the sheet of knn_cases.size_cases at the sizes the table asks for"""
    from tests import knn_cases as kc
    rng = np.random.default_rng([101, ns, nt])
    tgt = kc.surface(rng, nt)
    return dev(kc.surface(rng, ns, noise=0.003)), dev(tgt)


for _ns, _nt in ((1, 1), (257, 513), (1025, 2049)):
    @row("knn1_grid[%dx%d]" % (_ns, _nt), ["knn_grid"], ["gs_knn1_grid_scratch_bytes"])
    def _knn(ctx, ns=_ns, nt=_nt):
        src, tgt = _knn_clouds(ns, nt)
        ctx.expect("knn_grid", "gs_knn1_grid_scratch_bytes", ns, nt)
        return bits_of(ctx.ops.knn1_grid(src, tgt, return_unresolved=True))


# =========================================================================================== icp, icp_bwd
for _mode in (0, 1):
    @row("icp[mode%d]" % _mode, ["icp"], ["gs_icp_scratch_bytes"])
    def _icp(ctx, mode=_mode):
        from tests import test_hip_icp_one_driver as tod
        src, tgt, tn = tod._clouds(97, 12)
        ctx.expect("icp", "gs_icp_scratch_bytes", 97, 144)
        return bits_of(ctx.ops.icp(src, tgt, tn, mode=mode, numiters=3, return_trace=True))

    @row("icp_map[mode%d]" % _mode, ["icp"], ["gs_icp_scratch_bytes"])
    def _icp_map(ctx, mode=_mode):
        from tests import test_hip_icp_one_driver as tod
        s = tod._scene(97, 1)
        ctx.expect("icp", "gs_icp_scratch_bytes", 97, s["P"].shape[0])
        return bits_of(tod._single(ctx.ops, s, 97, 1, mode, 3))


for _det in (False, True):
    @row("icp_backward[%s]" % ("deterministic" if _det else "atomic"), ["icp", "icp_bwd"],
         ["gs_icp_scratch_bytes", "gs_icp_backward_scratch_bytes"])
    def _icp_bwd(ctx, det=_det):
        """the atomic mode adds float64 atomics in any order: its gradients are held to SUM_BOUND, the ordered mode's
        to equal bits (tests/test_icp_backward.py::test_deterministic_backward_is_bitwise_reproducible)"""
        from tests import test_hip_icp_one_driver as tod
        ctx.mp.setenv("GRADSLAM_HIP_DETERMINISTIC_BACKWARD", "1" if det else "0")
        src, tgt, tn = tod._clouds(97, 12)
        ctx.expect("icp", "gs_icp_scratch_bytes", 97, 144)
        ctx.expect("icp_bwd", "gs_icp_backward_scratch_bytes", 97, 144)
        T, idx, tape, prm = ctx.ops.icp_with_tape(src, tgt, tn, numiters=3)
        init = torch.eye(4, device="cuda")
        grads = ctx.ops.icp_backward(tape, prm, src, tgt, tn, init, dev(bc.weights((4, 4), 31)))
        assert all(bool(torch.isfinite(g).all()) for g in grads) and bool(grads[1].any())
        return bits_of([T, idx]) + (bits_of(grads, "grad") if det else sums_of(grads, "grad"))


# =========================================================================================== localize%d and its stats
for _H, _W in ((8, 11), (67, 131)):
    @row("localize_batch[%dx%d]" % (_H, _W), ["localize%d"], ["gs_localize_scratch_bytes"])
    def _localize(ctx, H=_H, W=_W):
        """B = 2, ds = 4; the stats exporters read what the solve left under the same name: the one documented hand-over,
        inside one context (they ask for the same size, so they log nothing)"""
        from tests import test_hip_icp_one_driver as tod
        s = tod._scene(H, W)
        rows = s["P"].shape[0]
        maps = [(s["P"], s["N"], rows, None)] * 2
        for b in range(2):
            ctx.expect("localize%d" % b, "gs_localize_scratch_bytes", H, W, 4, rows)
        two = lambda t: torch.stack([t, t])      # noqa: E731
        T = ctx.ops.localize_batch(two(s["vertex"]), two(s["depth"]), two(s["K"]), two(s["prev"]), maps, 4, mode=1, numiters=3)
        torch.cuda.synchronize()
        d = torch.device("cuda", torch.cuda.current_device())
        stats = [(ctx.ops.localize_list_stats(d, b, H, W, 4, rows), ctx.ops.localize_solve_stats(d, b, H, W, 4, rows))
                 for b in range(2)]
        assert bool(torch.isfinite(T).all()) and torch.equal(T[0], T[1])
        return bits_of(T) + bits_of([[list(x) for x in st[0]] + [st[1]["weak"]] for st in stats], "stats")


# =========================================================================================== map_update, map_update%d
# What these rows can see (checked by hand once with a sizer short by its gs_align(4 P) term): the sizer ends in a fixed
# 4096-byte pad, so at 24 x 40 (gs_align(4 * 960) = 3840) the short sizer still covers every write and only the 37 x 53
# single-sequence rows (7936 > 4096) trip, on the trailing guard.  The batched rows size by the store's capacity, n + H W
# rows, while the kernels index pix[] by the bound n: that slack hides a term of this size there.
def _update_scene(size):
    from tests import test_hip_update_fewer_gathers as ufg
    return ufg.built(size, "holes")[0]       # B = 2, maps of 300 and 1000 rows


for _size in sorted(FRAMES):
    for _b in (0, 1):
        @row("update_map_fusion_[%s-seq%d]" % (_size, _b), ["map_update"], ["gs_update_map_scratch_bytes"])
        def _update_one(ctx, size=_size, b=_b):
            from tests import test_hip_update_fewer_gathers as ufg
            sc = _update_scene(size)
            s = sc["seqs"][b]
            n = s["P"].shape[0]
            ctx.expect("map_update", "gs_update_map_scratch_bytes", n, sc["H"], sc["W"])
            bufs = ufg.store(s)
            res = ctx.ops.update_map_fusion_(*bufs, n, dev(s["vertex"]), dev(s["normal"]), dev(s["depth"]), dev(s["rgb"]),
                                             dev(s["alpha"]), dev(s["pose"]), dev(s["K"]), sc["dist_th"], sc["dot_th"])
            return bits_of(list(res) + bufs)

    @row("update_map_fusion_batch_[%s]" % _size, ["map_update%d"], ["gs_update_map_scratch_bytes"])
    def _update_batch(ctx, size=_size):
        from tests import test_hip_update_fewer_gathers as ufg
        sc = _update_scene(size)
        for b, s in enumerate(sc["seqs"]):      # (sized by the capacity of the store: n + H W rows)
            ctx.expect("map_update%d" % b, "gs_update_map_scratch_bytes", s["P"].shape[0] + sc["H"] * sc["W"], sc["H"], sc["W"])
        return bits_of(ufg.run_batch_entry(ctx.ops, sc, True))


# =========================================================================================== render%d, render_bwd%d
def _render(ctx, case, radius=None):
    from tests import render_backward_cases as rc
    c = rc.build(case)
    L = c.poses.shape[0]
    ctx.expect("render0", "gs_render_scratch_bytes", L, c.H, c.W)
    kw = dict(c.kw) if radius is None else dict(radius=radius)
    r = ctx.ops.render_map(dev(c.points), dev(c.normals), dev(c.colors), dev(c.ccounts), dev(c.poses), dev(c.K), c.H, c.W, **kw)
    assert int((r.index >= 0).sum()) > 1000
    return bits_of(tuple(r))


# the two smallest of test_hip_render.CASES, seq_pose and off_pose (the 96 x 128 map, one view, no filter), are the forwards
# of render_backward_cases r0_seq and, at radius 0, r1_off; views9: 9 views, three launches of at most 4
@row("render_map[seq_pose]", ["render%d"], ["gs_render_scratch_bytes"])
def _render_seq(ctx):
    return _render(ctx, "r0_seq")


@row("render_map[off_pose]", ["render%d"], ["gs_render_scratch_bytes"])
def _render_off(ctx):
    return _render(ctx, "r1_off", radius=0)


@row("render_map[views9]", ["render%d"], ["gs_render_scratch_bytes"])
def _render_views9(ctx):
    return _render(ctx, "views9")


def _render_backward(ctx, points_only):
    """r0_seq, the smallest case; two identical calls give equal bits (test_hip_render_backward)"""
    from tests import render_backward_cases as rc
    from tests.test_hip_render_backward import backward_through, upstream
    c = rc.build("r0_seq")
    ctx.expect("render0", "gs_render_scratch_bytes", 1, c.H, c.W)
    if not points_only:     # (the pose adjoint's partial rows are the only use of the backward's scratch)
        ctx.expect("render_bwd0", "gs_render_backward_scratch_bytes", 1, c.H, c.W, c.points.shape[0])
    leaves = [dev(a).requires_grad_(i == 0 or not points_only) for i, a in enumerate((c.points, c.normals, c.colors, c.ccounts))]
    P = dev(c.poses).requires_grad_(not points_only)
    r = ctx.ops.render_map(*leaves, P, dev(c.K), c.H, c.W, differentiable=True, **c.kw)
    backward_through((r.depth, r.color, r.normal, r.confidence), upstream(c))
    assert bool(leaves[0].grad.any())
    return bits_of([t.grad for t in leaves] + [P.grad])


@row("render_backward[all]", ["render%d", "render_bwd%d"], ["gs_render_scratch_bytes", "gs_render_backward_scratch_bytes"])
def _render_bwd_all(ctx):
    return _render_backward(ctx, False)


@row("render_backward[points_only]", ["render%d"], ["gs_render_scratch_bytes"])
def _render_bwd_points(ctx):
    return _render_backward(ctx, True)


# =========================================================================================== picp%d: every route
PICP_SHAPES = ((17, 31, 1, "cover"), (17, 31, 3, "special"), (60, 80, 4, "block"))    # 527 slots, 66 slots, 300 slots
WEIGHT = 0.2


def picp_routes():
    """{(family, export, sizer): (option set name, options, weights, tape, tables)}: per (export, sizer) pair that
    ops._picp_route can return for the forward families over GEO and JOINT, the configuration that reaches it with the
    most of weights, tape and tables on (the first of those in the order of the loops): return_weights next to pixel
    weights and a tape behind the robust, scaled and weighted entries run on exact buffers too"""
    from gradslam_amd import ops
    found = collections.OrderedDict()
    # (JOINT has no set with the geometric median rule alone, the one way to "color_scaled": GEO's "k" is added for it)
    joint = dict(JOINT, k=GEO["k"])
    for family, sets in (("batch", GEO), ("rows", GEO), ("color_batch", joint), ("color_rows", joint)):
        for which in sorted(sets):
            kw = dict(color_weight=WEIGHT, **sets[which]) if family.startswith("color") else dict(sets[which])
            opt = ops._picp_options("projective_icp", geometry=(1, 3, 1e-8, 0.1, 30.0), **kw)
            for weights in (False, True):
                for tape in ((False, True) if family == "batch" else (False,)):
                    for tables in ((False, True) if family.endswith("rows") else (False,)):
                        export, sizer = ops._picp_route(family, opt, weights=weights, tape=tape, tables=tables)
                        key, on = (family, export, sizer), weights + tape + tables
                        if key not in found or on > sum(found[key][2:]):
                            found[key] = (which, sets[which], weights, tape, tables)
    return found


def _picp_forward(ctx, family, export, sizer, kw, weights, tape, tables, h, w, stride, kind):
    from tests import test_hip_picp_weighted as tw
    ops = ctx.ops
    fx, wts = tw.fixture(h, w, kind, color=family.startswith("color"))
    numiters = 3
    ctx.expect("picp0", ops._PICP_SIZERS[sizer], h, w, stride)
    wt = dev(wts) if weights else None
    geo = tw.geo_args(fx)
    if family == "batch":
        opt = ops._picp_options("projective_icp", geometry=(stride, numiters, 1e-8, 0.1, 30.0), **kw)
        assert ops._picp_route(family, opt, weights=weights, tape=tape) == (export, sizer)
        b = lambda k: dev(fx[k]).unsqueeze(0)      # noqa: E731
        tapes = None
        if tape:     # the tape is the caller's buffer: guarded like the scratch
            nbytes = ctx.size("gs_projective_icp_tape_bytes", numiters)
            tapes = ctx.buffer("tape0", nbytes).view(1, nbytes)
        res = ops._picp_solve(opt, b("vertex"), b("normal"), b("depth"), b("K"), b("index"), b("model_pose"),
                              [(dev(fx["points"]), dev(fx["normals"]), None, None)], b("T0"), tapes=tapes,
                              weights=None if wt is None else [wt], return_trace=True, return_scale=True)
        assert float(res[1][0, -1, 0]) > 0        # (inliers of the last iteration)
    elif family == "rows":
        res = ops.projective_icp_rows(*geo, dev(fx["T0"]), stride=stride, pixel_weights=wt, return_weights=tables, **kw)
    elif family == "color_batch":
        res = ops.projective_icp_color(*geo, dev(fx["T0"]), *tw.color_args(fx), color_weight=WEIGHT, stride=stride,
                                       numiters=numiters, return_trace=True, return_scale=True, return_color_scale=True,
                                       pixel_weights=wt, **kw)
    else:
        res = ops.projective_icp_color_rows(*geo, dev(fx["T0"]), *tw.color_args(fx), color_weight=WEIGHT, stride=stride,
                                            pixel_weights=wt, return_weights=tables, **kw)
    return bits_of(res)


for (_family, _export, _sizer), (_which, _kw, _wts, _tape, _tables) in picp_routes().items():
    for _shape in PICP_SHAPES:
        _names = ["picp%d"]
        from gradslam_amd.ops import _PICP_SIZERS as _PS
        _sz = [_PS[_sizer]] + (["gs_projective_icp_tape_bytes"] if _tape else [])

        @row("picp[%s-%s-%dx%d-s%d]" % (_export, _sizer, _shape[0], _shape[1], _shape[2]), _names, _sz)
        def _picp(ctx, a=(_family, _export, _sizer, _kw, _wts, _tape, _tables) + _shape):
            return _picp_forward(ctx, *a)


for _B in (3, 9):
    @row("picp[weighted_batch-B%d]" % _B, ["picp%d"], ["gs_projective_icp_scaled_scratch_bytes"])
    def _picp_batch(ctx, B=_B):
        """B = 3 with the middle weights NULL; B = 9 past one launch group of 8 (60 x 80, stride 4, huber_k)"""
        from tests import test_hip_picp_weighted as tw
        seqs = tw.three_sequences()
        wts = tw.batch_weights(seqs)
        some = [seqs[i % 3] for i in range(B)]
        w = [None if i in (1, 7) else dev(wts[i % 3]) for i in range(B)]
        for b in range(B):
            ctx.expect("picp%d" % b, "gs_projective_icp_scaled_scratch_bytes", 60, 80, 4)
        T, trace = tw.batch_call(ctx.ops, some, w, stride=4, numiters=4, huber_k=tw.K_HUBER)
        assert bool((trace[:, -1, 0] > 20).all())
        return bits_of([T, trace])


# =========================================================================================== picp_bwd%d, picp_bwd_sort
BWD_MODES = {   # mode: (the case module's name, forward options, deterministic, weighted)
    "backward": ("picp_backward_cases", {}, False, False),
    "robust": ("picp_robust_backward_cases", "delta", False, False),
    "scaled": ("picp_scale_backward_cases", "k", False, False),
    "ordered": ("picp_backward_cases", {}, True, False),
    "weighted_atomic": ("picp_backward_cases", {}, False, True),
    "weighted_ordered": ("picp_backward_cases", {}, True, True),
}
WANT_MAPS = {"none": (False, False), "points": (True, False), "both": (True, True)}


def _picp_backward(ctx, mode, want, B):
    """edge_s3 (37 x 53, stride 3: 234 slots) and its robust and scaled siblings.  n_map of the sizer: the map's bound
    when a map output is asked for, else 0 -- ops._picp_backward and pb_backward must carve the same way.  vertex_bar,
    init_pose_bar and pixel_weights_bar are bitwise reproducible in both modes, the map gradients in the ordered mode;
    the atomic mode's are held to SUM_BOUND (test_hip_picp_backward.MAP_BOUND)"""
    import importlib
    from tests import picp_weighted_ref as wr
    ops = ctx.ops
    module, extra, det, weighted = BWD_MODES[mode]
    c = importlib.import_module("tests." + module).build("edge_s3")
    extra = dict(huber_delta=c.delta) if extra == "delta" else dict(huber_k=c.huber_k) if extra == "k" else {}
    fx, H, W = c.fx, c.fx["depth"].shape[0], c.fx["depth"].shape[1]
    st = lambda k: torch.stack([dev(fx[k])] * B)      # noqa: E731
    args = [st(k) for k in ("vertex", "normal", "depth", "K", "index", "model_pose")]
    n_rows = fx["points"].shape[0]
    maps = [(dev(fx["points"]), dev(fx["normals"]), None,
             None if c.device_count is None else torch.tensor([c.device_count], dtype=torch.int64, device="cuda"))
            for _ in range(B)]
    opt = ops._picp_options("projective_icp", geometry=(c.stride, c.numiters, c.kw["damp"], c.kw["dist_thresh"],
                                                        c.kw["angle_thresh"]), **extra)
    fwd_sizer = "gs_projective_icp_scaled_scratch_bytes" if "huber_k" in extra else "gs_projective_icp_scratch_bytes"
    nbytes = ctx.size("gs_projective_icp_tape_bytes", c.numiters)
    tapes = ctx.buffer("tapes", B * nbytes).view(B, nbytes)
    wts = torch.stack([dev(wr.random_weights((H, W), seed=20 + b)) for b in range(B)]) if weighted else None
    for b in range(B):
        ctx.expect("picp%d" % b, fwd_sizer, H, W, c.stride)
    ops._picp_solve(opt, *args, maps, st("T0"), tapes=tapes, weights=None if wts is None else list(wts))
    n_map = n_rows if any(WANT_MAPS[want]) else 0
    for b in range(B):
        if weighted:
            ctx.expect("picp_bwd%d" % b, "gs_projective_icp_weighted_backward_scratch_bytes", H, W, c.stride, n_map, int(det))
        else:
            ctx.expect("picp_bwd%d" % b, "gs_projective_icp_ordered_backward_scratch_bytes" if det else
                       "gs_projective_icp_backward_scratch_bytes", H, W, c.stride, n_map)
    if det and n_map:
        ctx.expect("picp_bwd_sort", "gs_projective_icp_ordered_backward_sort_scratch_bytes", B, H, W, c.stride)
    T_bar = torch.stack([dev(bc.weights((4, 4), 40 + b)) for b in range(B)])
    res = ops.projective_icp_backward_batch(*args, maps, tapes, T_bar, stride=c.stride, numiters=c.numiters, **c.kw,
                                            **extra, deterministic=det, want_maps=[WANT_MAPS[want]] * B,
                                            pixel_weights=wts, want_pixel_weights=weighted)
    vb, rows_out, ib = res[:3]
    assert bool(vb.any()) and bool(ib.any()) and (n_map == 0 or bool(rows_out[0][0].any()))
    out = bits_of([vb, ib], "pose_side") + (bits_of if det else sums_of)(rows_out, "map_side")
    return out + (bits_of(res[-1], "weights_bar") if weighted else [])


for _mode in BWD_MODES:
    for _want in WANT_MAPS:
        for _B in (1, 9):
            _det, _wtd = BWD_MODES[_mode][2], BWD_MODES[_mode][3]
            _sz = ["gs_projective_icp_tape_bytes",
                   "gs_projective_icp_scaled_scratch_bytes" if _mode == "scaled" else "gs_projective_icp_scratch_bytes",
                   "gs_projective_icp_weighted_backward_scratch_bytes" if _wtd else
                   "gs_projective_icp_ordered_backward_scratch_bytes" if _det else "gs_projective_icp_backward_scratch_bytes"]
            _nm = ["picp%d", "picp_bwd%d"]
            if _det and _want != "none":
                _sz.append("gs_projective_icp_ordered_backward_sort_scratch_bytes")
                _nm.append("picp_bwd_sort")

            @row("picp_backward[%s-%s-B%d]" % (_mode, _want, _B), _nm, _sz)
            def _pbwd(ctx, a=(_mode, _want, _B)):
                return _picp_backward(ctx, *a)


# =========================================================================================== picp_outliers%d
for _h, _w in ((5, 7), (37, 53)):
    for _weighted in (False, True):
        @row("picp_outliers[%dx%d%s]" % (_h, _w, "-weights" if _weighted else ""), ["picp_outliers%d"],
             ["gs_picp_outlier_classes_scratch_bytes"])
        def _outliers(ctx, h=_h, w=_w, weighted=_weighted):
            from tests import picp_ref as pr
            from tests import picp_weighted_ref as wr
            from tests.test_hip_outlier_mask import outliers_call
            fx = pr.convergence_fixture(h, w)
            ctx.expect("picp_outliers0", "gs_picp_outlier_classes_scratch_bytes", h, w)
            kw = dict(pixel_weights=dev(wr.random_weights((h, w)))) if weighted else {}
            return bits_of(outliers_call(ctx.ops, fx, fx["T0"], grow=2, min_support=2, **kw))


# =========================================================================================== prune%d, voxel%d
for _n in (1, 1023, 1024, 1025, 2049):
    @row("prune_map[%d]" % _n, ["prune%d"], ["gs_prune_scratch_bytes"])
    def _prune(ctx, n=_n):
        from tests import test_hip_prune as tp
        arrs = tp.rows(n)
        ctx.expect("prune0", "gs_prune_scratch_bytes", n)
        src = [dev(a) for a in arrs]
        out = [tp.sentinel((n + 7, a.shape[1])) for a in arrs]
        r = ctx.ops.prune_map_batch([tuple(src) + (n, None)], min_confidence=0.5, out=[out])
        return bits_of([r.maps, r.counts, r.removed])


for _n in (512, 513, 1025):
    @row("voxel_keep[%d]" % _n, ["voxel%d"], ["gs_voxel_keep_scratch_bytes"])
    def _voxel(ctx, n=_n):
        """the library compares scratch_bytes with its sizer: the exact size must be accepted"""
        from tests import test_hip_voxel as tv
        P, C = tv.fixture_data()
        ctx.expect("voxel0", "gs_voxel_keep_scratch_bytes", n)
        return bits_of(tv.run(ctx.ops, P[:n], C[:n]))


# =========================================================================================== kbar, pose_bar
@row("frame_maps_backward[kbar]", ["kbar"], ["gs_frame_maps_backward_kbar_scratch_bytes"])
def _kbar(ctx):
    depth, K = bc.frame_case(37, 53)
    ctx.expect("kbar", "gs_frame_maps_backward_kbar_scratch_bytes", 37, 53)
    d, k = dev(depth).requires_grad_(True), dev(K).requires_grad_(True)
    outs = ctx.ops.FrameMapsFunction.apply(d, k, SIGMA)
    torch.autograd.backward(outs, [dev(x) for x in bc.frame_weights(37, 53, "vna")])
    assert bool(k.grad.any())
    return bits_of([d.grad, k.grad])


@row("global_maps_backward[pose_bar]", ["pose_bar"], ["gs_global_maps_pose_backward_scratch_bytes"])
def _pose_bar(ctx):
    depth, K = bc.frame_case(37, 53)
    ctx.expect("pose_bar", "gs_global_maps_pose_backward_scratch_bytes", 37, 53)
    v, n, _, _ = ctx.ops.frame_maps(dev(depth), dev(K), SIGMA)
    v, n = v.clone().requires_grad_(True), n.clone().requires_grad_(True)
    pose = dev(bc.generic_pose()).requires_grad_(True)
    outs = ctx.ops.GlobalMapsFunction.apply(v, n, dev(depth), pose)
    torch.autograd.backward(outs, [dev(bc.weights((37, 53, 3), 1)), dev(bc.weights((37, 53, 3), 2))])
    assert bool(pose.grad.any())
    return bits_of([v.grad, n.grad, pose.grad])


# =========================================================================================== the drivers
DRIVERS = {    # row: (class, arguments, the workspace names its three steps use, whether the fast path serves them)
    "PointFusion-gradicp": ("PointFusion", dict(odom="gradicp"), ["localize%d", "map_update%d"], True),
    "PointFusion-icp": ("PointFusion", dict(odom="icp"), ["localize%d", "map_update%d"], True),
    "ICPSLAM": ("ICPSLAM", dict(), ["localize%d", "scratch"], False),
    "PointFusion-projicp": ("PointFusion", dict(odom="projicp"), ["picp%d", "render%d", "map_update%d"], False),
}
DRIVER_SIZERS = {"localize%d": "gs_localize_scratch_bytes", "map_update%d": "gs_update_map_scratch_bytes",
                 "scratch": "gs_scratch_bytes", "picp%d": "gs_projective_icp_scratch_bytes", "render%d": "gs_render_scratch_bytes"}


@functools.lru_cache(maxsize=None)
def _driver_frames():
    from gradslam_amd.datasets.synthetic import make_sequence
    return [make_sequence(3, 67, 131, seed=s) for s in (0, 1)]


def _drive(ctx, which):
    """B = 2, 67 x 131, 3 frames, in place (the fast path where the driver has one); the slam object and its StepPlan are
    created inside the context, so no pointer outlives it.  The arguments the row states: the first step reserves the
    map's buffers for several frames, so their capacity is one number per sequence over the three steps (asserted), and
    the localisation and the update size by it; the model view and the projective solve size by the frame.  ICPSLAM's
    append asks the shared "scratch" for gs_scratch_bytes(bound of the count before the step, H W), sequence after
    sequence: the expected log is those requests under the reuse rule (a request is logged when it outgrows the buffer)."""
    import gradslam_amd as gs
    from tests.test_hip_picp import frames_of
    cls, kw, names, fast = DRIVERS[which]
    H, W, ds = 67, 131, 4
    frames = frames_of(gs, _driver_frames())
    slam = getattr(gs.slam, cls)(dsratio=ds, numiters=4, device="cuda", **kw)
    pc, prev, poses, caps, bounds = gs.Pointclouds(device="cuda"), None, [], [], []
    for s in range(3):
        live = frames[:, s]
        bounds.append([0, 0] if len(pc) == 0 else [int(pc._count_of(b)[0]) for b in range(2)])
        pc, p = slam.step(pc, live, prev, inplace=True)
        live.poses = p
        prev = live
        poses.append(p[:, 0].clone())
        caps.append([int(pc._buf["points"][b].shape[0]) for b in range(2)])
    torch.cuda.synchronize()
    assert not fast or getattr(slam, "_step_plan", None) is not None, "the in-place loop must have taken the fast path"
    assert caps[0] == caps[1] == caps[2], caps
    for b, cap in enumerate(caps[0]):
        if "localize%d" in names:
            ctx.expect("localize%d" % b, "gs_localize_scratch_bytes", H, W, ds, cap)
        if "map_update%d" in names:
            ctx.expect("map_update%d" % b, "gs_update_map_scratch_bytes", cap, H, W)
        if "picp%d" in names:
            ctx.expect("picp%d" % b, "gs_projective_icp_scratch_bytes", H, W, ds)
        if "render%d" in names:
            ctx.expect("render%d" % b, "gs_render_scratch_bytes", 1, H, W)
    if "scratch" in names:
        have = -1
        for step in bounds:
            for n0 in step:
                want = ctx.size("gs_scratch_bytes", n0, H * W)
                if want > have:
                    ctx.expected.append(("scratch", want))
                    have = want
    assert all(t.shape[0] > 1000 for t in pc.points_list)
    maps = [[t[b] for t in (pc.points_list, pc.normals_list, pc.colors_list)] for b in range(2)]
    return bits_of([maps, poses, [t.shape[0] for t in pc.points_list]])


for _which in DRIVERS:
    @row("driver[%s]" % _which, DRIVERS[_which][2], [DRIVER_SIZERS[n] for n in DRIVERS[_which][2]])
    def _driver(ctx, which=_which):
        return _drive(ctx, which)


# =========================================================================================== the table itself
@gpu
@pytest.mark.parametrize("rid", [r.id for r in ROWS])
def test_row(ops, monkeypatch, rid):
    run_row({r.id: r for r in ROWS}[rid], ops, monkeypatch)


@gpu
def test_entries_without_scratch_log_no_request(ops, monkeypatch):
    """free_space_batch, bilateral_depth, ingest_frames_native, frame_maps and global_maps take no scratch: the day one of
    them does, it needs a row"""
    from tests import test_hip_carve as tc
    from tests.test_hip_ingest_stream import u16
    depth, K = bc.frame_case(37, 53)
    P, D, Ts = tc.fixture_data()
    raw_d = u16(np.full((2, 4, 6), 5000, np.uint16)).cuda()
    raw_c = torch.full((2, 4, 6, 3), 7, dtype=torch.uint8, device="cuda")
    with sg.exact_scratch(monkeypatch, 0xFF) as log:
        v, n, _, _ = ops.frame_maps(dev(depth), dev(K), SIGMA)
        ops.global_maps(v, n, dev(depth), dev(bc.generic_pose()))
        ops.bilateral_depth(dev(depth), radius=2)
        tc.run(ops, P[:300], None, D[:3], Ts[:3])       # (ops.free_space -> free_space_batch)
        ops.ingest_frames_native(raw_d, raw_c, torch.empty(48, device="cuda"), torch.empty(144, device="cuda"), 5000.0)
        torch.cuda.synchronize()
    assert sg.requests(log) == []


@gpu
def test_a_write_behind_a_real_scratch_is_reported(ops, monkeypatch):
    """the GPU path of the harness: one byte written with torch just behind the buffer a real knn1_grid call used"""
    src, tgt = _knn_clouds(257, 513)
    with sg.exact_scratch(monkeypatch, 0x7F) as log:
        ops.knn1_grid(src, tgt)
        torch.cuda.synchronize()
        assert sg.intact(log) == (True, [])
        (name, nbytes, outer), = log
        assert name == "knn_grid" and nbytes == _C.lib().gs_knn1_grid_scratch_bytes(257, 513)
        outer[sg.GUARD + nbytes] = 0x80
        assert sg.intact(log) == (False, [("knn_grid", "trailing", 0, 0)])
