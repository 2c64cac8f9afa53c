"""The map update of the one-call step (gs_pointfusion_step_batch_f32 with gvertex = gnormal = NULL) leaves out frame
gathers whose value it holds or can prove:

  A  the key pass asks for the pixel's normal first and gathers the vertex only for a row that passes the dot test;
  B  the merge computes the alpha of the winner's pixel from the local vertex it has loaded instead of gathering alpha[p];
  C  the merge reads best_pix[p] only in a frame in which the key pass marked a tie;
  D  the append computes alpha like B.

None of this may change a bit.  Every scene below goes through the step and through the explicit entry
(ops.update_map_fusion_batch_: global maps materialised, the caller's alpha map gathered), and both are held, without
tolerance, to each other and to the CPU oracle (oracle.associate + oracle.fuse_append through oracle.fusion_edges):
best_pix, the new row count, and every bit of points, normals, colours and confidence counts; rows behind the new count
stay untouched.

Images are 24 x 40 (960 pixels: less than one 1024-pixel tile) and 37 x 53 (1961 pixels: two tiles, no dimension a multiple
of a tile, a wave or the ICP lattice step).  Every call has B = 2 sequences with maps of 300 and 1000 rows (neither a
multiple of the 256-row block).  The frames have pixels without depth on the border, in a block inside and scattered, and a
far band whose alpha clamps to 1e-7."""
import numpy as np
import pytest
import torch

from oracle import fusion_edges as fe
from oracle import oracle as o
from tests import scratch_guard

gpu = pytest.mark.gpu
SIGMA, DIST_TH, DOT_TH, DS = 0.6, 0.05, 0.9, 4
SENTINEL = 7.25
SIZES = {"24x40": (24, 40), "37x53": (37, 53)}
ROWS = (300, 1000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------- scenes
def make_frame(H, W, seed):
    """a tilted, slightly bumpy surface; the right quarter of the image 2.5 m further away (alpha = exp(-|v|^2 / 0.72)
    falls below 1e-7 from |v| = 3.41 m on); no depth on the top row, the last column, a block inside and 4 % of the rest"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (1.5 + 0.01 * xx + 0.02 * yy + 0.002 * rng.rand(H, W)).astype(np.float32)
    depth[:, 3 * W // 4:] += np.float32(2.5)
    depth[rng.rand(H, W) < 0.04] = 0.0
    depth[0, :] = 0.0
    depth[:, W - 1] = 0.0
    depth[H // 3:H // 3 + 4, W // 4:W // 4 + 5] = 0.0
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = float(W)
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    a = 0.05
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    pose[:3, 3] = (0.1, -0.05, 0.2)
    vertex, normal, alpha, _ = o.frame_maps(depth, K, SIGMA)
    gvertex, gnormal = o.global_maps(vertex, normal, depth, pose)
    # pixels a row can be made to match: depth, and a normal of unit length (a pixel whose forward differences reach into a
    # hole has one too, but its length is whatever the hole made of it)
    good = (depth > 0) & (np.abs(np.linalg.norm(gnormal, axis=-1) - 1.0) < 1e-3)
    return dict(H=H, W=W, depth=depth, K=K, pose=pose, vertex=vertex, normal=normal, alpha=alpha, gvertex=gvertex, gnormal=gnormal,
                rgb=rng.rand(H, W, 3).astype(np.float32), good=np.flatnonzero(good.ravel()),
                holes=np.flatnonzero((depth <= 0).ravel()), rng=rng)


class Rows(object):
    """the map of one sequence, row by row"""

    def __init__(self, fr):
        self.fr, self.P, self.N, self.C, self.F = fr, [], [], [], []

    def _push(self, P, N, cc):
        self.P.append(np.asarray(P, np.float32))
        self.N.append(np.asarray(N, np.float32))
        self.C.append(self.fr["rng"].rand(3).astype(np.float32))
        self.F.append(np.float32(cc))
        return len(self.F) - 1

    def at(self, p, offset, cc, flip=False, along_ray=0.0):
        """a row on pixel p: the pixel's global vertex plus `offset` along its normal, moved by the fraction `along_ray` of
        its distance away from the camera (it stays on the pixel: 0.1 fails the distance test alone); the pixel's normal
        (flip: negated, fails the dot test)"""
        fr = self.fr
        gv, gn = fr["gvertex"].reshape(-1, 3)[p], fr["gnormal"].reshape(-1, 3)[p]
        c = fr["pose"][:3, 3]
        pt = gv + np.float32(offset) * gn
        pt = c + (pt - c) * np.float32(1.0 + along_ray)
        return self._push(pt, -gn if flip else gn, cc)

    def on_hole(self, p, cc):
        """a row that projects onto pixel p, which has no depth (global vertex and normal 0: both tests fail)"""
        fr = self.fr
        h, w = divmod(int(p), fr["W"])
        K, d = fr["K"], 2.0
        local = np.array([(w - K[0, 2]) / K[0, 0] * d, (h - K[1, 2]) / K[1, 1] * d, d], np.float32)
        return self._push(fr["pose"][:3, :3] @ local + fr["pose"][:3, 3], fr["pose"][:3, 2] * np.float32(-1.0), cc)

    def away(self, cc):
        """a row behind the camera: no pixel"""
        fr = self.fr
        return self._push(fr["pose"][:3, 3] - 3.0 * fr["pose"][:3, 2], (0, 0, 1), cc)

    def copy_of(self, i):
        """a row with every bit of row i's point, normal and confidence (the whole key), and a colour of its own"""
        return self._push(self.P[i], self.N[i], self.F[i])

    def fill(self, n, skip=(), matching=True):
        """ordinary rows up to n in all, several to a pixel: matching, dot test failed, distance test failed, both failed
        (as such and on a hole), behind the camera.  matching=False: none of the first kind"""
        fr, rng = self.fr, self.fr["rng"]
        pool = np.setdiff1d(fr["good"], np.asarray(skip, np.int64))
        while len(self.F) < n:
            r, p, cc = rng.rand(), pool[rng.randint(pool.size)], rng.randint(1, 4)
            off = (rng.rand() - 0.5) * 0.01
            if r < 0.08:
                self.away(cc)
            elif r < 0.20:
                self.on_hole(fr["holes"][rng.randint(fr["holes"].size)], cc)
            elif r < 0.32:
                self.at(p, off, cc, flip=True)
            elif r < 0.44:
                self.at(p, off, cc, along_ray=0.1)
            elif r < 0.52:
                self.at(p, off, cc, flip=True, along_ray=0.1)
            elif matching:
                self.at(p, off, cc)
        return self

    def seq(self):
        fr = self.fr
        s = {k: fr[k] for k in ("vertex", "normal", "gvertex", "gnormal", "alpha", "depth", "rgb", "pose", "K")}
        s.update(P=np.stack(self.P), N=np.stack(self.N), C=np.stack(self.C), F=np.asarray(self.F, np.float32).reshape(-1, 1))
        return s


def tie_pixel(fr):
    """a pixel for the hand-placed rows: a near one (its alpha is not clamped), in the middle of the good ones"""
    near = fr["good"][fr["alpha"].ravel()[fr["good"]] > 1e-6]
    return int(near[near.size // 2])


def make_scene(size, kind):
    H, W = SIZES[size]
    frames = [make_frame(H, W, 11), make_frame(H, W, 12)]
    seqs, winners = [], {}
    for b, (fr, n) in enumerate(zip(frames, ROWS)):
        r = Rows(fr)
        p0 = tie_pixel(fr)
        if kind == "all_new":
            while len(r.F) < n:           # nothing in the frame: the key pass turns every row away at the projection
                r.away(1 + len(r.F) % 3)
        elif kind == "none_matches" or (kind == "one_without_matches" and b == 0):
            r.fill(n, matching=False)     # rows in the frame, none similar: every one fails a test of the key pass
        elif kind in ("tie", "no_tie") and b == 1:
            # two rows with the same key on one pixel, of higher confidence than every other row, 517 rows (two blocks)
            # apart; in "no_tie" the second one is a row behind the camera instead
            r.fill(254, skip=(p0,))
            first = r.at(p0, 1e-3, 9.0)
            r.fill(771, skip=(p0,))
            if kind == "tie":
                assert r.copy_of(first) == 771
            else:
                r.away(9.0)
            r.fill(n, skip=(p0,))
            winners[(b, p0)] = first
        else:
            r.fill(n)
        seqs.append(r.seq())
    return dict(B=2, H=H, W=W, dist_th=DIST_TH, dot_th=DOT_TH, seqs=seqs), winners


KINDS = ("holes", "tie", "no_tie", "one_without_matches", "none_matches", "all_new")
_cache = {}


def built(size, kind):
    """scene, hand-written winners, oracle runs with and without renorm_all: computed once per case and left alone"""
    if (size, kind) not in _cache:
        sc, winners = make_scene(size, kind)
        _cache[(size, kind)] = (sc, winners, fe.oracle_scene(sc, True), fe.oracle_scene(sc, False))
    return _cache[(size, kind)]


def row_classes(sc, b, tabs):
    """per row of sequence b: in the frame, passes the dot test, passes the distance test (numpy, on the oracle's pixels)"""
    s, pix = sc["seqs"][b], tabs[b]["pix"]
    inf = pix >= 0
    gv, gn = s["gvertex"].reshape(-1, 3)[pix.clip(0)], s["gnormal"].reshape(-1, 3)[pix.clip(0)]
    dot = (gn * s["N"]).sum(-1) > DOT_TH
    dist = np.linalg.norm(gv - s["P"], axis=-1) < DIST_TH
    return inf, dot, dist


# ------------------------------------------------------------------------------------------- the two paths
def store(s):
    """capacity-backed copy of the map: n + H*W rows, a sentinel behind the map"""
    n, P = s["P"].shape[0], s["depth"].size
    bufs = []
    for k, w in zip("PNCF", (3, 3, 3, 1)):
        b = torch.full((n + P, w), SENTINEL, dtype=torch.float32, device="cuda")
        b[:n] = dev(s[k])
        bufs.append(b)
    return bufs


def run_batch_entry(ops, sc, renorm):
    stack = lambda k: dev(np.stack([s[k] for s in sc["seqs"]]))   # noqa: E731
    stores = [store(s) for s in sc["seqs"]]
    maps = [tuple(b) + (s["P"].shape[0], torch.tensor([s["P"].shape[0]], dtype=torch.int64, device="cuda"))
            for b, s in zip(stores, sc["seqs"])]
    cnt, _, _, best = ops.update_map_fusion_batch_(maps, stack("vertex"), stack("normal"), stack("depth"), stack("rgb"),
                                                   stack("alpha"), stack("pose"), stack("K"), sc["dist_th"], sc["dot_th"], renorm)
    cnt = host(cnt)
    return [(host(best[b]).ravel(), int(cnt[b]), [host(t) for t in stores[b]]) for b in range(sc["B"])]


def run_step_entry(ops, sc, renorm):
    """gs_pointfusion_step_batch_f32 on the frames' depth images, global maps implicit; numiters = 0: out_pose = prev_pose"""
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
    stores = [store(s) for s in sc["seqs"]]
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
        q.map = ops._map_view(bufs, cap, s["P"].shape[0], n_dev[b:])
        q.loc_scratch, q.upd_scratch = loc.data_ptr(), upd.data_ptr()
    prm = _C.IcpParams(1, 0, 1e-8, -1.0, 2.0, 1.0, 1.0, 200.0)
    _C.check(L.gs_pointfusion_step_batch_f32(seqs, B, H, W, DS, prm, ops.two_sigma_sq(SIGMA), float(sc["dist_th"]),
                                             float(sc["dot_th"]), 1 if renorm else 0, _C.stream(depth.device)),
             "gs_pointfusion_step_batch_f32")
    torch.cuda.synchronize()
    ok, hits = scratch_guard.intact(guards)
    assert ok, ("the step wrote outside a scratch of exactly the sizer's size", hits)
    # the step made the frame maps itself and updated under the pose it wrote: they must be the scene's, and the alpha map
    # -- which the update no longer reads -- is still written, every bit
    for b, s in enumerate(sc["seqs"]):
        fe.same_bits(host(out_pose[b]), s["pose"], "step pose", signed_zero=False)
        fe.same_bits(host(vertex[b]), s["vertex"], "step vertex map", signed_zero=False)
        fe.same_bits(host(normal[b]), s["normal"], "step normal map", signed_zero=False)
        fe.same_bits(host(alpha[b]), s["alpha"], "step alpha map")
    cnt = host(cnt)
    return [(host(best[b]).ravel(), int(cnt[b]), [host(t) for t in stores[b]]) for b in range(B)]


def check(got, want, what):
    """best_pix, the new count and rows [0, count) bit for bit; whatever lies behind the new count untouched"""
    for b, ((best, cnt, bufs), t) in enumerate(zip(got, want)):
        w = "%s[%d]" % (what, b)
        fe.same_bits(best, t["best"], w + " best_pix")
        assert cnt == t["fP"].shape[0], (w, "new row count", cnt, t["fP"].shape[0])
        for h, k in zip(bufs, ("fP", "fN", "fC", "fF")):
            fe.same_bits(h[:cnt], t[k], "%s %s" % (w, k))
            assert (h[cnt:] == SENTINEL).all(), "%s %s: rows beyond the new count were written" % (w, k)


def as_tables(run):
    return [dict(best=best, fP=bufs[0][:cnt], fN=bufs[1][:cnt], fC=bufs[2][:cnt], fF=bufs[3][:cnt]) for best, cnt, bufs in run]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_step_update_equals_explicit_entry_and_oracle(ops, size, kind):
    sc, winners, tabs, tabs_fast = built(size, kind)
    for (b, p), row in winners.items():   # the winner written down by hand: the oracle agrees before anything is held to it
        assert tabs[b]["best"][p] == row, (size, kind, b, p, row, tabs[b]["best"][p])
    for renorm, tt in ((True, tabs), (False, tabs_fast)):
        w = "%s %s (renorm_all=%s)" % (size, kind, renorm)
        explicit = run_batch_entry(ops, sc, renorm)
        check(explicit, tt, "explicit entry vs oracle, " + w)
        step = run_step_entry(ops, sc, renorm)
        check(step, tt, "one-call step vs oracle, " + w)
        check(step, as_tables(explicit), "one-call step vs explicit entry, " + w)


# ------------------------------------------------------------------------------------------- the scenes are what they claim
@pytest.mark.parametrize("size", sorted(SIZES))
def test_scenes_say_what_they_claim(size):
    H, W = SIZES[size]
    assert (H * W <= 1024) == (size == "24x40") and all(n % 256 for n in ROWS)
    sc, _, tabs, _ = built(size, "holes")
    for b, s in enumerate(sc["seqs"]):
        assert s["P"].shape[0] == ROWS[b]
        d = s["depth"]
        assert (d[0] == 0).all() and (d[:, -1] == 0).all() and (d[1:-1, 1:-1] == 0).sum() >= 20   # holes: border and inside
        inf, dot, dist = row_classes(sc, b, tabs)
        for name, m in (("dot test only", inf & ~dot & dist), ("distance test only", inf & dot & ~dist),
                        ("both tests", inf & ~dot & ~dist), ("neither", inf & dot & dist), ("not in the frame", ~inf)):
            assert m.sum() >= 10, (size, b, "rows that fail: " + name, int(m.sum()))
        assert np.array_equal(inf & dot & dist, tabs[b]["sim"].astype(bool))
        on_hole = inf & (d.ravel()[tabs[b]["pix"].clip(0)] <= 0)
        assert on_hole.sum() >= 10 and not (dot | dist)[on_hole].any()        # a row on a hole fails both
        # alpha clamped to 1e-7: under winners (the merge) and under new pixels (the append); unclamped ones under both too
        a, best = s["alpha"].ravel(), tabs[b]["best"]
        new = (d.ravel() > 0) & (best < 0)
        for m, what in ((best >= 0, "merged"), (new, "appended")):
            assert (a[m] == np.float32(1e-7)).sum() >= 5 and (a[m] > np.float32(1e-6)).sum() >= 5, (size, b, what)
    # the tie: two rows of sequence 1 with the same key bits on one pixel, the lower index wins; sequence 0 of the same call
    # and the whole "no_tie" scene have no two competing rows with equal keys (the merge's non-reading branch)
    for kind, want in (("tie", [0, 1]), ("no_tie", [0, 0])):
        sc, winners, tabs, _ = built(size, kind)
        (b1, p0), first = list(winners.items())[0]
        for b, s in enumerate(sc["seqs"]):
            sim, pix = tabs[b]["sim"].astype(bool), tabs[b]["pix"]
            d = s["P"] - s["gvertex"].reshape(-1, 3)[pix.clip(0)]
            ray = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]   # float32, the key's order of operations
            keys, ties = set(), 0
            for i in np.flatnonzero(sim):   # same pixel, same 1 / (count + 1e-20) and same squared distance: the same key
                k = (int(pix[i]), s["F"][i, 0].tobytes(), ray[i].tobytes())
                ties += k in keys
                keys.add(k)
            assert ties == want[b], (size, kind, b, ties)
        assert b1 == 1 and first == 254 and tabs[1]["best"][p0] == 254
        if kind == "tie":
            s = sc["seqs"][1]
            assert all(np.array_equal(s[k][254], s[k][771]) for k in "PNF") and not np.array_equal(s["C"][254], s["C"][771])
    sc, _, tabs, _ = built(size, "one_without_matches")
    assert [bool((t["best"] >= 0).any()) for t in tabs] == [False, True]
    assert (tabs[0]["pix"] >= 0).sum() > 100                  # ... its rows are in the frame and fail the tests
    for kind in ("none_matches", "all_new"):
        sc, _, tabs, _ = built(size, kind)
        assert not any((t["best"] >= 0).any() for t in tabs)  # call_flag stays 0
        for s, t in zip(sc["seqs"], tabs):                    # every pixel with depth is new: only the append writes
            assert t["fP"].shape[0] == s["P"].shape[0] + int((s["depth"] > 0).sum())
            fe.same_bits(t["fP"][:s["P"].shape[0]], s["P"], kind + ": old rows untouched")
    assert not any((t["pix"] >= 0).any() for t in built(size, "all_new")[2])
