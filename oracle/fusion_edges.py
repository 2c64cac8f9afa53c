"""Reader of tests/golden/fusion_edges.npz (written by oracle/make_golden_fusion_edges.py) and the C oracle's run of one
of its scenes.  TEST INFRASTRUCTURE ONLY: shared by the generator's own oracle-equals-reference assertion, by
tests/test_fusion_edges_cpu.py and by tests/test_hip_fusion_edges.py.

A scene is a batch of B sequences that go through ONE map update.  Per sequence the file holds the inputs (map P / N / C /
F, the reference's local and global vertex / normal maps, alpha, depth, rgb, pose, K) and the reference's outputs (active
rows, similar mask, unique rows, fused P / N / C / F), under the keys "<scene>/<field>": the B arrays joined along axis 0, their lengths in
"<scene>/len"."""
import numpy as np

from oracle import oracle as o

IN_FIELDS = ("P", "N", "C", "F", "vertex", "normal", "gvertex", "gnormal", "alpha", "depth", "rgb", "pose", "K")
OUT_FIELDS = ("active", "similar_mask", "unique", "fP", "fN", "fC", "fF")


def scene_names(g):
    return [str(s) for s in g["scenes"]]


def load_scene(g, name):
    """-> dict(name, B, H, W, dist_th, dot_th, ref (False: the reference cannot run the scene, outputs are the oracle's),
    seqs = [dict of IN_FIELDS + OUT_FIELDS (+ expect_pix where the pixel of every row was written down by hand)])"""
    B, H, W, ref = (int(x) for x in g[name + "/meta"])
    dist_th, dot_th = (float(x) for x in g[name + "/th"])
    fields = IN_FIELDS + OUT_FIELDS + (("expect_pix",) if name + "/expect_pix" in g.files else ())
    seqs = [dict() for _ in range(B)]
    for k, lens in zip(fields, g[name + "/len"]):   # one array per field: the sequences' arrays joined along axis 0
        for s, a in zip(seqs, np.split(g[name + "/" + k], np.cumsum(lens)[:-1], 0)):
            s[k] = np.ascontiguousarray(a)
    return dict(name=name, B=B, H=H, W=W, dist_th=dist_th, dot_th=dot_th, ref=bool(ref), seqs=seqs)


def same_bits(a, b, what="", signed_zero=True):
    """Bit-for-bit, sign of zero included; a NaN equals a NaN (depth NaN / inf scenes carry them through).
    signed_zero=False: +0 and -0 compare equal (the contract of test_hip_parity.py for the frame and global maps: a pixel
    without depth is v * 0, whose sign follows the operation order of the rotation)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        if not signed_zero:
            ok |= (a == 0) & (b == 0)
    else:
        ok = a == b
    if not ok.all():
        first = np.argwhere(~ok)[0]
        raise AssertionError("%s: %d of %d differ, first at %s: %r vs %r" % (
            what, (~ok).sum(), ok.size, tuple(int(i) for i in first), a[tuple(first)], b[tuple(first)]))


def oracle_tables(s, H, W, dist_th, dot_th):
    """C oracle of the association of one sequence, fed the reference's global maps."""
    pix = o.project_map(s["P"], s["pose"], s["K"], H, W)
    act = o.active_table(pix, W)
    mask = o.similar_rows(act, s["P"], s["N"], s["gvertex"], s["gnormal"], dist_th, dot_th)
    uq = o.best_unique_rows(act[mask], s["P"], s["F"], s["gvertex"])
    best, sim = o.associate(pix, s["P"], s["N"], s["F"], s["gvertex"], s["gnormal"], dist_th, dot_th)
    return dict(pix=pix, active=act, similar_mask=mask, unique=uq, best=best, sim=sim)


def oracle_scene(sc, renorm_all=True):
    """C oracle of the whole scene -> per sequence dict(pix, active, similar_mask, unique, best, sim, fP, fN, fC, fF).
    The reference's merge is skipped only when NO sequence of the batch has a match (fusionutils.py:659)."""
    H, W = sc["H"], sc["W"]
    tabs = [oracle_tables(s, H, W, sc["dist_th"], sc["dot_th"]) for s in sc["seqs"]]
    batch_any = any((t["best"] >= 0).any() for t in tabs)
    for s, t in zip(sc["seqs"], tabs):
        assert np.array_equal(o.best_table(t["best"], H, W), t["unique"])
        assert np.array_equal(o.rows_to_best_pix(t["unique"], H, W), t["best"])
        assert np.array_equal(t["sim"][t["pix"] >= 0], t["similar_mask"]) and not t["sim"][t["pix"] < 0].any()
        mode = (2 if batch_any else 1) if renorm_all else 0
        t["fP"], t["fN"], t["fC"], t["fF"] = o.fuse_append(s["P"], s["N"], s["C"], s["F"], t["best"], s["gvertex"],
                                                         s["gnormal"], s["rgb"], s["alpha"], s["depth"], mode)
    return tabs


def rows_of(table, b):
    """rows of sequence b of a (R, 4) [b, n, h, w] table, with the batch index set to 0 (the oracle's single sequence)"""
    r = table[table[:, 0] == b].copy()
    r[:, 0] = 0
    return r


def assert_oracle_is_reference(sc, tabs):
    """Indices, masks and counts bit-exact; fused values bit-exact (the oracle was fed the reference's alpha and maps)."""
    for b, (s, t) in enumerate(zip(sc["seqs"], tabs)):
        w = "%s[%d]" % (sc["name"], b)
        if "expect_pix" in s:
            same_bits(t["pix"], s["expect_pix"], w + " pix (by hand)")
        same_bits(t["active"], s["active"], w + " active")
        same_bits(t["similar_mask"], s["similar_mask"], w + " similar")
        same_bits(t["unique"], s["unique"], w + " unique")
        assert t["fP"].shape[0] == s["fP"].shape[0], (w, "count", t["fP"].shape[0], s["fP"].shape[0])
        for k in ("fP", "fN", "fC", "fF"):
            same_bits(t[k], s[k], w + " " + k)
