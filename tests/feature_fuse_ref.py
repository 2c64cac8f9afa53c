"""The feature-layer rule (include/gradslam_hip.h, "feature layers") restated in NumPy: the specification the HIP pass
gs_fuse_features_batch and the compaction gs_compact_features_batch are held to, bit for bit.

Every float32 operation is one NumPy float32 operation (one rounding each, no FMA); a float16 layer is converted to
float32, merged, and stored with `astype(float16)` (round to nearest even)."""
import numpy as np

f32 = np.float32


def rows_of_pixels(best_pix, depth, n_old):
    """row(p) for every pixel in raster order, -1 for none: best_pix[p] when 0 <= best_pix[p] < n_old; n_old + rank(p)
    when best_pix[p] < 0 and depth[p] > 0 (rank: such pixels before p; best_pix None: every pixel with depth); a stale
    entry >= n_old (and the tie marker) is none.  Returns (row_of_pix int32 (H * W,), new count)."""
    depth = np.asarray(depth, f32).reshape(-1)
    P = depth.shape[0]
    bp = np.full(P, -1, np.int32) if best_pix is None else np.asarray(best_pix, np.int32).reshape(-1)
    with np.errstate(invalid="ignore"):
        new = (bp < 0) & (depth > 0)
    matched = (bp >= 0) & (bp < n_old)
    rows = np.full(P, -1, np.int32)
    rows[matched] = bp[matched]
    rows[new] = n_old + np.arange(int(new.sum()), dtype=np.int64)
    return rows, int(n_old) + int(new.sum())


def fuse(emb, weight, n_old, best_pix, depth, alpha, feat, valid=None):
    """One frame's pass on copies of the layer (emb (capacity, C) float32 | float16, weight (capacity,) float32).
    feat: (H, W, C) of the layer's dtype or None (no pixel is valid); valid: (H * W,) uint8 / bool or None (every pixel).
    Returns (emb, weight, row_of_pix, n_new); rows at or beyond n_new are as they were."""
    emb, weight = np.array(emb, copy=True), np.array(weight, dtype=f32, copy=True)
    C = emb.shape[1]
    rows, n_new = rows_of_pixels(best_pix, depth, n_old)
    assert n_new <= emb.shape[0]
    P = rows.shape[0]
    alpha = np.asarray(alpha, f32).reshape(-1)
    if feat is None:
        val = np.zeros(P, bool)
    else:
        feat = np.asarray(feat).reshape(P, C)
        assert feat.dtype == emb.dtype
        val = np.ones(P, bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    has = rows >= 0
    matched = has & (rows < n_old)
    app = has & ~matched
    # appended rows
    pa, ra = np.nonzero(app & val)[0], rows[app & val]
    emb[ra] = feat[pa] if pa.size else emb[ra]
    weight[ra] = alpha[pa]
    rz = rows[app & ~val]
    emb[rz] = 0
    weight[rz] = f32(0.0)
    # matched rows (one pixel each)
    pm, rm = np.nonzero(matched & val)[0], rows[matched & val]
    if pm.size:
        assert np.unique(rm).size == rm.size, "a map row matched by two pixels"
        w = weight[rm]
        a = alpha[pm]
        w2 = w + a
        inv = f32(1.0) / np.where(w2 == f32(0.0), f32(1.0), w2)
        e = emb[rm].astype(f32)
        f = feat[pm].astype(f32)
        out = ((w[:, None] * e) + (a[:, None] * f)) * inv[:, None]
        assert out.dtype == f32
        emb[rm] = out.astype(emb.dtype)
        weight[rm] = w2
    return emb, weight, rows, n_new


def compact(emb, weight, keep, n):
    """Stable compaction of the first n rows by keep: survivor k becomes row k, bit for bit.  Returns (emb_rows,
    weight_rows, count) holding the survivors only."""
    k = np.asarray(keep[:n]) != 0
    return np.array(emb[:n][k], copy=True), np.array(weight[:n][k], copy=True), int(k.sum())


def keep_of_rule(conf, n, keep=None, min_confidence=None, young_from=None):
    """The map prune's selection over the first n rows: (keep is None or keep[r] != 0) and (min_confidence is None or
    r >= young_from or conf[r] >= float32(min_confidence)); a NaN confidence fails."""
    s = np.ones(n, bool) if keep is None else np.asarray(keep[:n]) != 0
    if min_confidence is not None:
        with np.errstate(invalid="ignore"):
            ok = np.asarray(conf[:n], f32) >= f32(min_confidence)
        if young_from is not None:
            ok |= np.arange(n) >= young_from
        s &= ok
    return s
