"""The map update on constructed edge scenes, against the REAL reference (tests/golden/fusion_edges.npz, recorded by
oracle/make_golden_fusion_edges.py) and the C oracle on the same inputs.

Every scene goes through every path that serves it -- the table-level kernels, associate (host and device counts),
update_map_fusion_ and update_map_fusion_batch_ -- and all of them must give the same best_pix, count and map bits.
Bars (headers of test_hip_parity.py / test_hip_api.py): indices, masks, tables and counts bit-exact against the golden;
fused values bit-exact against the C oracle (sign of zero included) and within rtol 1e-6 of the golden (colours atol 1e-4).
Kernels that take alpha and the global maps get the reference's; the fused entries make the global maps themselves, and
those are first held to the golden's bits (+0 = -0, as test_hip_parity.py compares the frame and global maps: the kernel's
FMA chain gives -0.0 on some pixels whose normal is 0 where the reference's einsum gives +0.0; first seen in general_ragged
at pixel (34, 95))."""
import numpy as np
import pytest
import torch

from oracle import fusion_edges as fe
from oracle import oracle as o

pytestmark = pytest.mark.gpu

SINGLE = ["borders", "borders_kzero", "borders_perm", "general_ragged", "general_dense", "thresholds", "thresholds_nodepth",
          "ties", "ties_one_mark", "ties_no_mark", "merge", "merge_nomatch", "append_all_new", "append_none_new",
          "append_last_tile", "append_first_only", "append_last_only", "tiny_1x1", "tiny_2x2"]
BATCH = ["batch9", "batch9_late", "batch2_one_empty_table"]
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scenes(golden):
    """name -> (scene, oracle run with renorm_all, oracle run without, hand-written winners or None); computed once"""
    g = golden("fusion_edges")
    cache = {}

    def get(name):
        if name not in cache:
            sc = fe.load_scene(g, name)
            hand = g[name + "/expect_best"] if name + "/expect_best" in g.files else None
            cache[name] = (sc, fe.oracle_scene(sc, True), fe.oracle_scene(sc, False), hand)
        return cache[name]
    return get


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def store(s, extra=0):
    """capacity-backed copy of the map: exactly n + extra + H*W rows, the free space filled with a sentinel"""
    n, P = s["P"].shape[0], s["depth"].size
    bufs = []
    for k, w in zip("PNCF", (3, 3, 3, 1)):
        b = torch.full((n + extra + P, w), SENTINEL, dtype=torch.float32, device="cuda")
        b[:n] = dev(s[k])
        bufs.append(b)
    return bufs


def check_map(bufs, cnt, s, t, what, golden=True, n_free_from=None):
    """rows [0, cnt) bit-exact against the oracle's, within the reference's bar of the golden's; the rest untouched"""
    cnt = int(cnt)
    assert cnt == t["fP"].shape[0] == (s["fP"].shape[0] if golden else cnt), (what, cnt, t["fP"].shape[0], s["fP"].shape[0])
    for b, k in zip(bufs, ("fP", "fN", "fC", "fF")):
        h = host(b)
        fe.same_bits(h[:cnt], t[k], "%s %s vs oracle" % (what, k))
        if golden:
            np.testing.assert_allclose(h[:cnt], s[k], rtol=1e-6, atol=1e-4 if k == "fC" else 0, equal_nan=True,
                                       err_msg="%s %s vs reference" % (what, k))
        assert (h[max(cnt, n_free_from or 0):] == SENTINEL).all(), "%s %s: rows beyond the new count were written" % (what, k)


def check_tables(best, s, t, hand, what):
    fe.same_bits(host(best).ravel(), t["best"], what + " best_pix vs oracle")
    H, W = s["depth"].shape
    fe.same_bits(o.best_table(host(best).ravel(), H, W), s["unique"], what + " best_pix vs reference")
    if hand is not None:
        fe.same_bits(host(best).ravel(), hand, what + " best_pix vs the winners written down by hand")


def frame_dev(s):
    return {k: dev(s[k]) for k in ("vertex", "normal", "gvertex", "gnormal", "alpha", "depth", "rgb", "pose", "K")}


def run_table_level(ops, sc, s, t, t_fast, hand, batch_any, what):
    H, W = sc["H"], sc["W"]
    n = s["P"].shape[0]
    P, N, C, F = (dev(s[k]) for k in "PNCF")
    f = frame_dev(s)
    pix = ops.project_map(P, f["pose"], f["K"], H, W)
    fe.same_bits(host(pix), t["pix"], what + " pix")
    if "expect_pix" in s:
        fe.same_bits(host(pix), s["expect_pix"], what + " pix vs the pixels written down by hand")
    best = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    if n > 0:
        act = ops.active_table(pix, W)
        fe.same_bits(host(act), s["active"], what + " active")
        if act.shape[0] > 0:
            mask = ops.similar_rows(act, P, N, f["gvertex"], f["gnormal"], sc["dist_th"], sc["dot_th"])
            fe.same_bits(host(mask), s["similar_mask"], what + " similar")
            if int(mask.sum()) > 0:
                uq, best = ops.best_unique_rows(act[mask], P, F, f["gvertex"])
                fe.same_bits(host(uq), s["unique"], what + " unique")
                fe.same_bits(host(ops.rows_to_best_pix(uq, H, W)), t["best"], what + " rows_to_best_pix")
        else:
            assert s["similar_mask"].size == 0
    else:
        assert s["active"].shape[0] == 0
    assert s["unique"].shape[0] == int((t["best"] >= 0).sum())
    check_tables(best, s, t, hand, what + " table level")
    fe.same_bits(host(ops.best_table(best, H, W)), s["unique"], what + " best_table")
    for n_dev in (None, torch.tensor([n], dtype=torch.int64, device="cuda")):
        b2, sim = ops.associate(pix, P, N, F, f["gvertex"], f["gnormal"], sc["dist_th"], sc["dot_th"], want_similar=True,
                                n_dev=n_dev)
        check_tables(b2, s, t, hand, what + " associate")
        fe.same_bits(host(sim), t["sim"], what + " associate similar")
    for renorm, tt in ((True, t), (False, t_fast)):
        bufs = store(s)
        mode = (2 if batch_any else 1) if renorm else 0
        cnt = ops.fuse_append_(*bufs, n, best, f["gvertex"], f["gnormal"], f["rgb"], f["alpha"], f["depth"], mode)
        check_map(bufs, cnt, s, tt, "%s fuse_append_(renorm_all=%d)" % (what, mode), golden=renorm)
    check_fast_mode_against_golden(s, t_fast, what)


def check_fast_mode_against_golden(s, t_fast, what):
    """renorm_all = False has no reference run: matched rows and appended rows are the golden's (the oracle's bits are
    within its bar), unmatched rows keep their input bits"""
    n = s["P"].shape[0]
    matched = np.zeros(n, bool)
    matched[s["unique"][:, 1]] = True
    for k, fk in zip("PNCF", ("fP", "fN", "fC", "fF")):
        fe.same_bits(t_fast[fk][:n][~matched], s[k][~matched], what + " fast mode: unmatched rows of " + k)
        sel = np.concatenate([matched, np.ones(s[fk].shape[0] - n, bool)])
        np.testing.assert_allclose(t_fast[fk][sel], s[fk][sel], rtol=1e-6, atol=1e-4 if k == "C" else 0, equal_nan=True)


def check_global_maps(gv, gn, s, what):
    fe.same_bits(host(gv), s["gvertex"], what + " global vertex map vs reference", signed_zero=False)
    fe.same_bits(host(gn), s["gnormal"], what + " global normal map vs reference", signed_zero=False)


def run_single_entry(ops, sc, s, t, hand, renorm, what, extra=0, n_dev=None, bufs=None):
    n = s["P"].shape[0]
    f = frame_dev(s)
    bufs = store(s, extra) if bufs is None else bufs
    nd = torch.tensor([n if n_dev is None else n_dev], dtype=torch.int64, device="cuda")
    cnt, gv, gn, best = ops.update_map_fusion_(*bufs, n + extra, f["vertex"], f["normal"], f["depth"], f["rgb"], f["alpha"],
                                               f["pose"], f["K"], sc["dist_th"], sc["dot_th"], renorm, n_dev=nd)
    check_global_maps(gv, gn, s, what)
    return bufs, int(host(cnt)[0]), best


def run_batch_entry(ops, sc, renorm):
    Bn = sc["B"]
    stack = lambda k: dev(np.stack([s[k] for s in sc["seqs"]]))   # noqa: E731
    stores = [store(s) for s in sc["seqs"]]
    maps = [tuple(b) + (s["P"].shape[0], None if i % 2 else torch.tensor([s["P"].shape[0]], dtype=torch.int64, device="cuda"))
            for i, (b, s) in enumerate(zip(stores, sc["seqs"]))]   # host and device counts, alternating
    cnt, gv, gn, best = ops.update_map_fusion_batch_(maps, stack("vertex"), stack("normal"), stack("depth"), stack("rgb"),
                                                     stack("alpha"), stack("pose"), stack("K"), sc["dist_th"], sc["dot_th"],
                                                     renorm)
    assert cnt.shape[0] == Bn
    return stores, host(cnt), gv, gn, best


def check_batch(ops, scenes, name):
    sc, tabs, tabs_fast, hand = scenes(name)
    for renorm, tt in ((True, tabs), (False, tabs_fast)):
        stores, cnt, gv, gn, best = run_batch_entry(ops, sc, renorm)
        for b, (s, t) in enumerate(zip(sc["seqs"], tt)):
            what = "%s[%d] batch entry (renorm_all=%s)" % (name, b, renorm)
            check_global_maps(gv[b], gn[b], s, what)
            check_tables(best[b], s, t, hand, what)
            check_map(stores[b], cnt[b], s, t, what, golden=renorm)


# ------------------------------------------------------------------------------------------- every scene, every path
@pytest.mark.parametrize("name", SINGLE)
def test_single_sequence_scene_through_every_path(ops, scenes, name):
    sc, tabs, tabs_fast, hand = scenes(name)
    s, t, tf = sc["seqs"][0], tabs[0], tabs_fast[0]
    run_table_level(ops, sc, s, t, tf, hand, False, name)
    for renorm, tt in ((True, t), (False, tf)):
        what = "%s update_map_fusion_(renorm_all=%s)" % (name, renorm)
        bufs, cnt, best = run_single_entry(ops, sc, s, tt, hand, renorm, what)
        check_tables(best, s, tt, hand, what)
        check_map(bufs, cnt, s, tt, what, golden=renorm)
    check_batch(ops, scenes, name)   # the batch entry at B = 1


@pytest.mark.parametrize("name", BATCH)
def test_batch_scene_through_every_path(ops, scenes, name):
    sc, tabs, tabs_fast, _ = scenes(name)
    batch_any = any((t["best"] >= 0).any() for t in tabs)
    assert batch_any
    for b, (s, t, tf) in enumerate(zip(sc["seqs"], tabs, tabs_fast)):
        run_table_level(ops, sc, s, t, tf, None, batch_any, "%s[%d]" % (name, b))
    check_batch(ops, scenes, name)


def test_merge_with_alpha_zero_at_table_level(ops, scenes):
    """alpha == 0 cannot come out of the reference's get_alpha (clamped to 1e-7): against the oracle alone"""
    sc, tabs, _, _ = scenes("merge")
    s = dict(sc["seqs"][0], alpha=np.zeros_like(sc["seqs"][0]["alpha"]))
    f = frame_dev(s)
    for renorm in (1, 0):
        want = dict(zip(("fP", "fN", "fC", "fF"), o.fuse_append(s["P"], s["N"], s["C"], s["F"], tabs[0]["best"], s["gvertex"],
                                                                s["gnormal"], s["rgb"], s["alpha"], s["depth"], renorm)))
        bufs = store(s)
        cnt = ops.fuse_append_(*bufs, s["P"].shape[0], dev(tabs[0]["best"]), f["gvertex"], f["gnormal"], f["rgb"], f["alpha"],
                               f["depth"], renorm)
        check_map(bufs, cnt, s, want, "merge with alpha 0 (renorm_all=%d)" % renorm, golden=False)


# ------------------------------------------------------------------------------------------- rows behind the device count
@pytest.mark.parametrize("name", ["ties", "general_dense"])
def test_poisoned_rows_behind_the_device_count(ops, scenes, name):
    """Rows [n_dev, n_bound) hold copies of the winners with ccount 1e20: they would win every pixel if read."""
    sc, tabs, _, hand = scenes(name)
    s, t = sc["seqs"][0], tabs[0]
    H, W, n = sc["H"], sc["W"], s["P"].shape[0]
    winners = s["unique"][:, 1]
    extra = winners.size

    def poisoned():
        bufs = store(s, extra)
        for b, k in zip(bufs, "PNCF"):
            b[n:n + extra] = dev(s[k][winners] if k != "F" else np.full((extra, 1), 1e20, np.float32))
        return bufs
    bufs = poisoned()
    before = [host(b).copy() for b in bufs]
    f = frame_dev(s)
    nd = torch.tensor([n], dtype=torch.int64, device="cuda")
    pix = ops.project_map(bufs[0][:n + extra], f["pose"], f["K"], H, W, n_dev=nd)
    fe.same_bits(host(pix)[:n], t["pix"], name + " project_map(n_dev)")
    pix_all = ops.project_map(bufs[0][:n + extra], f["pose"], f["K"], H, W)   # (every row projected: the poison is live)
    assert (host(pix_all)[n:] >= 0).all()
    best, sim = ops.associate(pix_all, bufs[0][:n + extra], bufs[1][:n + extra], bufs[3][:n + extra], f["gvertex"], f["gnormal"],
                              sc["dist_th"], sc["dot_th"], want_similar=True, n_dev=nd)
    check_tables(best, s, t, hand, name + " associate(n_dev)")
    fe.same_bits(host(sim)[:n], t["sim"], name + " associate(n_dev) similar")
    cnt = ops.fuse_append_(*bufs, n + extra, best, f["gvertex"], f["gnormal"], f["rgb"], f["alpha"], f["depth"], True, n_dev=nd)

    def check(bufs, cnt, what):
        assert int(cnt) == t["fP"].shape[0]
        for b, b0, k in zip(bufs, before, ("fP", "fN", "fC", "fF")):
            h = host(b)
            fe.same_bits(h[:cnt], t[k], "%s %s" % (what, k))
            fe.same_bits(h[cnt:], b0[cnt:], "%s %s: rows behind the new count" % (what, k))
    check(bufs, cnt, name + " fuse_append_(n_dev)")
    bufs = poisoned()
    bufs, cnt, best = run_single_entry(ops, sc, s, t, hand, True, name + " update_map_fusion_(n_dev < n_bound)", extra=extra,
                                       n_dev=n, bufs=bufs)
    check_tables(best, s, t, hand, name + " update_map_fusion_(n_dev < n_bound)")
    check(bufs, cnt, name + " update_map_fusion_(n_dev < n_bound)")


def test_device_count_zero_under_a_positive_bound(ops, scenes):
    sc, _, _, _ = scenes("ties")
    s = sc["seqs"][0]
    n = s["P"].shape[0]
    e3, e1 = np.zeros((0, 3), np.float32), np.zeros((0, 1), np.float32)
    empty = dict(s, P=e3, N=e3, C=e3, F=e1)
    t = fe.oracle_scene(dict(sc, seqs=[empty]))[0]
    bufs = store(s)
    before = [host(b).copy() for b in bufs]
    bufs, cnt, best = run_single_entry(ops, sc, s, t, None, True, "n_dev = 0", n_dev=0, bufs=bufs)
    assert (host(best) == -1).all() and cnt == t["fP"].shape[0]
    for b, b0, k in zip(bufs, before, ("fP", "fN", "fC", "fF")):
        fe.same_bits(host(b)[:cnt], t[k], "n_dev = 0 " + k)
        fe.same_bits(host(b)[cnt:], b0[cnt:], "n_dev = 0 %s: rows behind the new count" % k)
    f = frame_dev(s)
    nd = torch.zeros(1, dtype=torch.int64, device="cuda")
    P, N, F = dev(s["P"]), dev(s["N"]), dev(s["F"])
    pix = ops.project_map(P, f["pose"], f["K"], sc["H"], sc["W"])
    best = ops.associate(pix, P, N, F, f["gvertex"], f["gnormal"], sc["dist_th"], sc["dot_th"], n_dev=nd)
    assert (host(best) == -1).all()
    bufs = store(s)
    cnt = ops.fuse_append_(*bufs, n, best, f["gvertex"], f["gnormal"], f["rgb"], f["alpha"], f["depth"], True, n_dev=nd)
    assert cnt == t["fP"].shape[0]
    for b, k in zip(bufs, ("fP", "fN", "fC", "fF")):
        fe.same_bits(host(b)[:cnt], t[k], "fuse_append_(n_dev = 0) " + k)


# ------------------------------------------------------------------------------------------- state carried in the workspace
def test_workspace_state_does_not_leak_between_calls(ops, scenes):
    for name in ("ties", "merge_nomatch", "ties", "ties_no_mark", "ties_one_mark"):
        sc, tabs, _, hand = scenes(name)
        s, t = sc["seqs"][0], tabs[0]
        bufs, cnt, best = run_single_entry(ops, sc, s, t, hand, True, name + " (repeated calls)")
        check_tables(best, s, t, hand, name + " (repeated calls)")
        check_map(bufs, cnt, s, t, name + " (repeated calls)")
    for name in ("batch9", "batch2_one_empty_table", "batch9_late", "merge_nomatch", "batch9"):
        check_batch(ops, scenes, name)


# ------------------------------------------------------------------------------------------- down-samplers
@pytest.mark.parametrize("name", ["general_ragged", "borders"])
@pytest.mark.parametrize("ds", [1, 2, 3, 4, 5, 8])
def test_downsamplers_against_the_oracle(ops, scenes, name, ds):
    from gradslam_amd import _C
    sc, tabs, _, _ = scenes(name)
    s, t = sc["seqs"][0], tabs[0]
    H, W = sc["H"], sc["W"]
    P, N, C = (dev(s[k]) for k in "PNC")
    f = frame_dev(s)
    pix = dev(t["pix"])
    want = o.select_targets(t["pix"], W, ds, s["P"], s["N"], s["C"])
    for got, w in zip(ops.select_targets(pix, W, ds, P, N, C), want):
        fe.same_bits(host(got), w, "select_targets ds=%d" % ds)
    for got, w in zip(ops.downsample_table(dev(t["active"]), ds, P, N, C), want):
        fe.same_bits(host(got), w, "downsample_table ds=%d" % ds)
    for got, w in zip(ops.downsample_frame(f["gvertex"], f["gnormal"], f["rgb"], f["depth"], ds),
                      o.downsample_frame(s["gvertex"], s["gnormal"], s["rgb"], s["depth"], ds)):
        fe.same_bits(host(got), w, "downsample_frame ds=%d" % ds)
    # lattice_source: the lattice pixels' global vertices (the reference's bits), NaN where the pixel has no depth
    lat = host(ops.lattice_source(f["vertex"], f["depth"], f["pose"], ds))
    want_lat = s["gvertex"][::ds, ::ds].reshape(-1, 3).copy()
    want_lat[~(s["depth"][::ds, ::ds].ravel() > 0)] = np.nan
    fe.same_bits(lat, want_lat, "lattice_source ds=%d" % ds)
    # cap below the survivor count: the count reports the total, rows up to cap are right, the rest is not written
    total = want[0].shape[0]
    cap = total // 2
    if cap == 0:
        return
    n = t["pix"].shape[0]
    outs = [torch.full((total, 3), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3)]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = _C.Workspace.get(pix.device)
    _C.check(_C.lib().gs_select_targets_f32(_C.ptr(pix), n, W, ds, _C.ptr(P), _C.ptr(N), _C.ptr(C), _C.ptr(outs[0]),
                                            _C.ptr(outs[1]), _C.ptr(outs[2]), cap, _C.ptr(cnt), _C.ptr(ws.scratch(n, 0)),
                                            _C.stream(pix.device)), "gs_select_targets_f32")
    assert int(host(cnt)[0]) == total
    for got, w in zip(outs, want):
        fe.same_bits(host(got)[:cap], w[:cap], "select_targets with cap")
        assert (host(got)[cap:] == SENTINEL).all(), "select_targets wrote beyond cap"


# ------------------------------------------------------------------------------------------- compaction beyond one scan block
def test_active_table_beyond_1024_tiles(ops):
    n, W = 1024 * 1025 + 3, 640
    i = np.arange(n, dtype=np.int64)
    keep = (i % 37 == 0) | ((i // 1024) % 129 == 5) | (i >= n - 2)     # sparse, with full tiles and the last rows
    pix = np.where(keep, (i * 7919) % (480 * W), -1).astype(np.int32)
    rows = host(ops.active_table(dev(pix), W, b=3))
    idx = np.nonzero(pix >= 0)[0]
    want = np.stack([np.full(idx.size, 3, np.int64), idx, pix[idx] // W, pix[idx] % W], 1)
    fe.same_bits(rows, want, "active_table")
