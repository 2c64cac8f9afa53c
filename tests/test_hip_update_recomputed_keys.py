"""The one-call map update keeps no per-row copy of the association key: the merge and the tie settling compute the key of
a row again (high word from the confidence count, low word from the pixel's global vertex) and the merge stores a
confidence count only when its bits change.  Scenes built here with numpy aim at what that can get wrong; every scene goes
through

  * ops.update_map_fusion_batch_ (global maps materialised by the update's pixel pass) and
  * gs_pointfusion_step_batch_f32 with gvertex = gnormal = NULL (the one-call step: the global vertex of a pixel is computed
    where it is used; numiters = 0, so the pose of the update is the previous pose),

and both must give, bit for bit and without any tolerance, what

  * the table-level kernels (ops.project_map -> ops.associate -> ops.fuse_append_, which keep their stored keys) and
  * the CPU oracle (oracle.oracle, as tests/test_hip_fusion_edges.py runs it)

give on the same inputs: best_pix, the new count and every bit of the map."""
import numpy as np
import pytest
import torch

from oracle import fusion_edges as fe
from oracle import oracle as o
from tests import scratch_guard

gpu = pytest.mark.gpu
SIGMA, DIST_TH, DOT_TH, DS = 0.6, 0.05, 0.9, 4
SENTINEL = 7.25


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------- scenes
def make_frame(H, W, seed):
    """a tilted, slightly bumpy surface seen by a camera a little off the origin; a few pixels without depth"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (1.5 + 0.01 * xx + 0.02 * yy + 0.002 * rng.rand(H, W)).astype(np.float32)
    depth[rng.rand(H, W) < 0.05] = 0.0
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = float(W)
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    a = 0.05
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    pose[:3, 3] = (0.1, -0.05, 0.2)
    vertex, normal, alpha, _ = o.frame_maps(depth, K, SIGMA)
    gvertex, gnormal = o.global_maps(vertex, normal, depth, pose)
    good = (depth > 0) & (np.abs(gnormal).sum(-1) > 0.5)
    good[[0, -1], :] = False
    good[:, [0, -1]] = False
    return dict(H=H, W=W, depth=depth, K=K, pose=pose, vertex=vertex, normal=normal, alpha=alpha, gvertex=gvertex, gnormal=gnormal,
                rgb=rng.rand(H, W, 3).astype(np.float32), good=np.flatnonzero(good.ravel()), rng=rng)


class Rows(object):
    """the map of one sequence, row by row"""

    def __init__(self, fr):
        self.fr, self.P, self.N, self.C, self.F, self.want_pix = fr, [], [], [], [], []

    def at(self, p, offset, cc, flip=False):
        """a row that projects to pixel p: the pixel's global vertex plus `offset` along its normal, its normal (negated:
        not similar), confidence count cc"""
        fr = self.fr
        gv, gn = fr["gvertex"].reshape(-1, 3)[p], fr["gnormal"].reshape(-1, 3)[p]
        self.P.append((gv + np.float32(offset) * gn).astype(np.float32))
        self.N.append(-gn if flip else gn)
        self.C.append(fr["rng"].rand(3).astype(np.float32))
        self.F.append(np.float32(cc))
        self.want_pix.append(int(p))
        return len(self.F) - 1

    def away(self, cc):
        """a row behind the camera: no pixel, no correspondence"""
        fr = self.fr
        self.P.append((fr["pose"][:3, 3] - 3.0 * fr["pose"][:3, 2]).astype(np.float32))
        self.N.append(np.array([0, 0, 1], np.float32))
        self.C.append(fr["rng"].rand(3).astype(np.float32))
        self.F.append(np.float32(cc))
        self.want_pix.append(-1)
        return len(self.F) - 1

    def fill(self, n, skip=()):
        """ordinary rows up to n in all: random pixels (several rows per pixel: different confidence, now and then the
        same), random small distances, one in eight not similar, one in eight away"""
        fr, rng = self.fr, self.fr["rng"]
        pool = np.setdiff1d(fr["good"], np.asarray(skip, np.int64))
        while len(self.F) < n:
            r = rng.rand()
            if r < 0.125:
                self.away(rng.randint(1, 4))
            else:
                self.at(pool[rng.randint(pool.size)], (rng.rand() - 0.5) * 0.01, rng.randint(1, 4), flip=r < 0.25)
        return self

    def seq(self):
        fr = self.fr
        s = {k: fr[k] for k in ("vertex", "normal", "gvertex", "gnormal", "alpha", "depth", "rgb", "pose", "K")}
        s.update(P=np.stack(self.P), N=np.stack(self.N).astype(np.float32), C=np.stack(self.C),
                 F=np.asarray(self.F, np.float32).reshape(-1, 1), want_pix=np.asarray(self.want_pix, np.int32))
        pix = o.project_map(s["P"], fr["pose"], fr["K"], fr["H"], fr["W"])
        assert np.array_equal(pix, s["want_pix"]), "scene construction: a row does not project where it was put"
        return s


def scene(fr, seqs):
    return dict(B=len(seqs), H=fr["H"], W=fr["W"], dist_th=DIST_TH, dot_th=DOT_TH, seqs=seqs)


def pixels(fr, k):
    return [int(p) for p in fr["good"][:: max(1, fr["good"].size // (k + 1))][:k]]


def case_high_word_ties(H, W, n):
    """three rows on one pixel, the same confidence bits, distances 3, 1 and 2 mm: the nearest (the second) wins, and the
    high word of the key cannot tell them apart"""
    fr = make_frame(H, W, 1)
    p0, p1 = pixels(fr, 2)
    r = Rows(fr).fill(n // 3, skip=(p0, p1))
    a = [r.at(p0, d, 2.0) for d in (3e-3, 1e-3, 2e-3)]
    b = [r.at(p1, d, 5.0) for d in (-2e-3, -3e-3, -1e-3)]     # a second trio, higher confidence than every other row
    s = r.fill(n, skip=(p0, p1)).seq()
    return scene(fr, [s]), {p0: a[1], p1: b[2]}


def case_full_ties(H, W, n, rows):
    """three identical rows (the same point, the same confidence: every bit of the key) at the given indices: the lowest
    index wins"""
    fr = make_frame(H, W, 2)
    p0 = pixels(fr, 1)[0]
    r = Rows(fr)
    for i in sorted(rows):
        r.fill(i, skip=(p0,))
        assert r.at(p0, 1e-3, 3.0) == i
    return scene(fr, [r.fill(n, skip=(p0,)).seq()]), {p0: min(rows)}


def case_zero_confidence(H, W, n):
    """ccounts = 0 (key 1 / 1e-20): alone on a pixel it wins, against a row with confidence 1 it loses; -0.0 likewise"""
    fr = make_frame(H, W, 3)
    p0, p1, p2, p3 = pixels(fr, 4)
    r = Rows(fr).fill(n // 2, skip=(p0, p1, p2, p3))
    a = r.at(p0, 1e-3, 0.0)
    r.at(p1, 1e-3, 0.0)
    b = r.at(p1, 2e-3, 1.0)
    c = r.at(p2, 1e-3, -0.0)
    r.at(p3, 1e-3, 0.0)            # +0 and -0 give the same key: the nearer one wins
    d = r.at(p3, 5e-4, -0.0)
    return scene(fr, [r.fill(n, skip=(p0, p1, p2, p3)).seq()]), {p0: a, p1: b, p2: c, p3: d}


def case_negative_zero_unmatched(H, W, n):
    """unmatched rows with ccounts = -0.0f: -0 + 0 = +0, the one unmatched row whose count changes bits"""
    fr = make_frame(H, W, 4)
    p0 = pixels(fr, 1)[0]
    r = Rows(fr).fill(n // 2, skip=(p0,))
    r.away(-0.0)
    r.at(p0, 1e-3, -0.0, flip=True)    # in the frame, not similar
    r.at(p0, 2e-3, -0.0)               # competes and loses
    w = r.at(p0, 1e-3, 2.0)
    return scene(fr, [r.fill(n, skip=(p0,)).seq()]), {p0: w}


def case_batch_flag(H, W, n, none_matches=False):
    """three sequences, the middle one without any correspondence (rows away or not similar): the batch-level "any match"
    flag decides whether its rows are renormalised"""
    fr = make_frame(H, W, 5)
    seqs = []
    for b in range(3):
        r = Rows(fr)
        if b == 1 or none_matches:
            for i in range(n + b):
                if i % 2:
                    r.away(1 + i % 3)
                else:
                    r.at(fr["good"][i % fr["good"].size], 1e-3, 1 + i % 3, flip=True)
        else:
            r.fill(n + b)
        seqs.append(r.seq())
    return scene(fr, seqs), {}


def case_rows(H, W, n):
    fr = make_frame(H, W, 6)
    return scene(fr, [Rows(fr).fill(n).seq()]), {}


CASES = {
    "high_word_ties": lambda: case_high_word_ties(12, 16, 40),
    "high_word_ties_24x32": lambda: case_high_word_ties(24, 32, 600),
    "full_ties_one_block": lambda: case_full_ties(12, 16, 300, (10, 100, 200)),
    "full_ties_across_blocks": lambda: case_full_ties(24, 32, 600, (255, 256, 400)),
    "zero_confidence": lambda: case_zero_confidence(12, 16, 64),
    "negative_zero_unmatched": lambda: case_negative_zero_unmatched(12, 16, 48),
    "batch_one_without_matches": lambda: case_batch_flag(12, 16, 90),
    "batch_none_matches": lambda: case_batch_flag(12, 16, 41, none_matches=True),
    "rows_257": lambda: case_rows(24, 32, 257),
    "rows_513": lambda: case_rows(24, 32, 513),
}


# ------------------------------------------------------------------------------------------- the four paths
def store(s, extra=0, poison=False):
    """capacity-backed copy of the map: n + extra + H*W rows; the `extra` rows behind the map are NaN (poison) or, like the
    free space, a sentinel"""
    n, P = s["P"].shape[0], s["depth"].size
    bufs = []
    for k, w in zip("PNCF", (3, 3, 3, 1)):
        b = torch.full((n + extra + P, w), SENTINEL, dtype=torch.float32, device="cuda")
        b[:n] = dev(s[k])
        if poison:
            b[n:n + extra] = float("nan")
        bufs.append(b)
    return bufs


def run_table_level(ops, sc, renorm, batch_any, extra):
    out = []
    for s in sc["seqs"]:
        H, W, n = sc["H"], sc["W"], s["P"].shape[0]
        bufs = store(s, extra, poison=True)
        nd = torch.tensor([n], dtype=torch.int64, device="cuda") if extra else None
        f = {k: dev(s[k]) for k in ("gvertex", "gnormal", "alpha", "depth", "rgb", "pose", "K")}
        pix = ops.project_map(bufs[0][:n + extra], f["pose"], f["K"], H, W, n_dev=nd)
        best = ops.associate(pix, bufs[0][:n + extra], bufs[1][:n + extra], bufs[3][:n + extra], f["gvertex"], f["gnormal"],
                             sc["dist_th"], sc["dot_th"], n_dev=nd)
        mode = (2 if batch_any else 1) if renorm else 0
        cnt = ops.fuse_append_(*bufs, n + extra, best, f["gvertex"], f["gnormal"], f["rgb"], f["alpha"], f["depth"], mode, n_dev=nd)
        out.append((host(best).ravel(), int(cnt), [host(b) for b in bufs]))
    return out


def run_batch_entry(ops, sc, renorm, extra):
    stack = lambda k: dev(np.stack([s[k] for s in sc["seqs"]]))   # noqa: E731
    stores = [store(s, extra, poison=True) for s in sc["seqs"]]
    maps = [tuple(b) + (s["P"].shape[0] + extra, torch.tensor([s["P"].shape[0]], dtype=torch.int64, device="cuda") if extra or i % 2
                        else None) for i, (b, s) in enumerate(zip(stores, sc["seqs"]))]
    cnt, _, _, best = ops.update_map_fusion_batch_(maps, stack("vertex"), stack("normal"), stack("depth"), stack("rgb"),
                                                   stack("alpha"), stack("pose"), stack("K"), sc["dist_th"], sc["dot_th"], renorm)
    cnt = host(cnt)
    return [(host(best[b]).ravel(), int(cnt[b]), [host(t) for t in stores[b]]) for b in range(sc["B"])]


def run_step_entry(ops, sc, renorm, extra):
    """gs_pointfusion_step_batch_f32 on the frame's depth image, global maps implicit; numiters = 0: out_pose = prev_pose"""
    from gradslam_amd import _C
    L = _C.lib()
    B, H, W = sc["B"], sc["H"], sc["W"]
    P = H * W
    stack = lambda k: dev(np.stack([s[k] for s in sc["seqs"]]))   # noqa: E731
    depth, rgb, K, prev = stack("depth"), stack("rgb"), stack("K"), stack("pose")
    f32 = torch.float32
    vertex, normal = torch.empty((B, H, W, 3), dtype=f32, device="cuda"), torch.empty((B, H, W, 3), dtype=f32, device="cuda")
    alpha, out_pose = torch.empty((B, H, W), dtype=f32, device="cuda"), torch.zeros((B, 4, 4), dtype=f32, device="cuda")
    best = torch.empty((B, P), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int64, device="cuda")
    stores = [store(s, extra, poison=True) for s in sc["seqs"]]
    n_dev = dev(np.array([s["P"].shape[0] for s in sc["seqs"]], np.int64))
    seqs = (_C.StepSeq * B)()
    guards = scratch_guard.GuardLog(0xFF)
    for b, (s, bufs) in enumerate(zip(sc["seqs"], stores)):
        cap = int(bufs[0].shape[0])
        # exactly what the sizers say, between guard bands, poisoned with 0xFF (tests/scratch_guard.py)
        loc = scratch_guard.guarded_buffer(guards, "loc_scratch%d" % b, L.gs_localize_scratch_bytes(H, W, DS, cap), "cuda")
        upd = scratch_guard.guarded_buffer(guards, "upd_scratch%d" % b, L.gs_update_map_scratch_bytes(cap, H, W), "cuda")
        q = seqs[b]
        q.depth, q.rgb, q.K16 = depth[b].data_ptr(), rgb[b].data_ptr(), K[b].data_ptr()
        q.prev_pose16, q.out_pose16 = prev[b].data_ptr(), out_pose[b].data_ptr()
        q.vertex, q.normal, q.alpha = vertex[b].data_ptr(), normal[b].data_ptr(), alpha[b].data_ptr()
        q.gvertex = q.gnormal = None
        q.best_pix, q.new_count_out = best[b].data_ptr(), cnt[b:].data_ptr()
        q.map = ops._map_view(bufs, cap, s["P"].shape[0] + extra, n_dev[b:])
        q.loc_scratch, q.upd_scratch = loc.data_ptr(), upd.data_ptr()
    prm = _C.IcpParams(1, 0, 1e-8, -1.0, 2.0, 1.0, 1.0, 200.0)
    _C.check(L.gs_pointfusion_step_batch_f32(seqs, B, H, W, DS, prm, ops.two_sigma_sq(SIGMA), float(sc["dist_th"]),
                                             float(sc["dot_th"]), 1 if renorm else 0, _C.stream(depth.device)),
             "gs_pointfusion_step_batch_f32")
    torch.cuda.synchronize()
    ok, hits = scratch_guard.intact(guards)
    assert ok, ("the step wrote outside a scratch of exactly the sizer's size", hits)
    # the step made the frame maps itself and updated under the pose it wrote: they must be the scene's
    for b, s in enumerate(sc["seqs"]):
        fe.same_bits(host(out_pose[b]), s["pose"], "step pose", signed_zero=False)
        fe.same_bits(host(vertex[b]), s["vertex"], "step vertex map", signed_zero=False)
        fe.same_bits(host(normal[b]), s["normal"], "step normal map", signed_zero=False)
        fe.same_bits(host(alpha[b]), s["alpha"], "step alpha")
    cnt = host(cnt)
    return [(host(best[b]).ravel(), int(cnt[b]), [host(t) for t in stores[b]]) for b in range(B)]


def check(got, want, sc, extra, what):
    """best_pix, count and rows [0, count) bit for bit; whatever lies behind the new count untouched"""
    for b, ((best, cnt, bufs), t, s) in enumerate(zip(got, want, sc["seqs"])):
        w = "%s[%d]" % (what, b)
        n = s["P"].shape[0]
        fe.same_bits(best, t["best"], w + " best_pix")
        assert cnt == t["fP"].shape[0], (w, cnt, t["fP"].shape[0])
        for h, k in zip(bufs, ("fP", "fN", "fC", "fF")):
            fe.same_bits(h[:cnt], t[k], "%s %s" % (w, k))
            tail = h[cnt:]
            behind = np.isnan(tail[:max(n + extra - cnt, 0)]).all() and (tail[max(n + extra - cnt, 0):] == SENTINEL).all()
            assert behind, "%s %s: rows beyond the new count were written" % (w, k)


def as_tables(run):
    return [dict(best=best, fP=bufs[0][:cnt], fN=bufs[1][:cnt], fC=bufs[2][:cnt], fF=bufs[3][:cnt]) for best, cnt, bufs in run]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


_cache = {}


def built(name):
    """scene, hand-written winners, oracle runs with and without renorm_all: computed once per case"""
    if name not in _cache:
        sc, winners = CASES[name]()
        _cache[name] = (sc, winners, fe.oracle_scene(sc, True), fe.oracle_scene(sc, False))
    return _cache[name]


def run_case(ops, name, extra=0):
    sc, winners, tabs, tabs_fast = built(name)
    for p, row in winners.items():   # the winners written down by hand: the oracle agrees before anything is held to it
        assert tabs[0]["best"][p] == row, (name, p, row, tabs[0]["best"][p])
    batch_any = any((t["best"] >= 0).any() for t in tabs)
    for renorm, tt in ((True, tabs), (False, tabs_fast)):
        table = run_table_level(ops, sc, renorm, batch_any, extra)
        check(table, tt, sc, extra, "%s table level vs oracle (renorm_all=%s)" % (name, renorm))
        for path, run in (("batch entry", run_batch_entry), ("one-call step", run_step_entry)):
            got = run(ops, sc, renorm, extra)
            check(got, tt, sc, extra, "%s %s vs oracle (renorm_all=%s)" % (name, path, renorm))
            check(got, as_tables(table), sc, extra, "%s %s vs table level (renorm_all=%s)" % (name, path, renorm))
    return sc, tabs


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_through_both_one_call_paths(ops, name):
    run_case(ops, name)


def test_scenes_say_what_they_claim():
    """the constructed situations are really there: rows that tie the winner's high word without winning, a sequence
    without matches next to sequences with some, unmatched rows whose count is -0.0"""
    sc, winners, tabs, _ = built("high_word_ties")
    s, best = sc["seqs"][0], tabs[0]["best"]
    for p, row in winners.items():
        tied = [i for i in np.flatnonzero(s["want_pix"] == p) if s["F"][i, 0] == s["F"][row, 0] and tabs[0]["sim"][i]]
        assert len(tied) == 3 and best[p] == row
    _, _, tabs, _ = built("batch_one_without_matches")
    assert [bool((t["best"] >= 0).any()) for t in tabs] == [True, False, True]
    _, _, tabs, _ = built("batch_none_matches")
    assert not any((t["best"] >= 0).any() for t in tabs)
    sc, _, tabs, _ = built("negative_zero_unmatched")
    F, fF = sc["seqs"][0]["F"], tabs[0]["fF"]
    unmatched = np.setdiff1d(np.arange(F.shape[0]), tabs[0]["best"][tabs[0]["best"] >= 0])
    neg = [i for i in unmatched if F[i, 0] == 0 and np.signbit(F[i, 0])]
    assert len(neg) == 3 and not np.signbit(fF[neg, 0]).any()   # -0 + 0 = +0: the stored bits change


@gpu
@pytest.mark.parametrize("name", ["full_ties_across_blocks", "high_word_ties"])
def test_poisoned_rows_behind_the_device_count(ops, name):
    """the host bound is 7 rows above the device count and those rows are NaN: no path may read or write them"""
    run_case(ops, name, extra=7)


def test_update_scratch_lost_the_per_row_keys():
    """gs_update_map_scratch_bytes, from which Python sizes the workspace: at least 8 bytes per row less than the layout
    that kept an 8-byte key per map row (written out here as it was)"""
    from gradslam_amd import _C
    n, H, W = 1 << 20, 480, 640
    al = lambda x: (x + 255) // 256 * 256   # noqa: E731
    P = H * W
    tiles = (P + 1023) // 1024
    before = 256 + al(8 * P) + al(4 * tiles) + al(8 * n) + 2 * al(4 * n) + 4096
    now = _C.lib().gs_update_map_scratch_bytes(n, H, W)
    assert 0 < now <= before - 8 * n, (now, before)
    assert now >= 256 + al(8 * P) + al(4 * tiles) + al(4 * n)   # key_pix, tile counts and pix[] are still there
