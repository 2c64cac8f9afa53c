"""NumPy restatement of the voxel thinning (gradslam_amd/csrc/gs_voxel.hip -> gs_voxel_keep_dc_f32 ->
ops.voxel_keep_batch -> Pointclouds.voxel_downsample_): a float32 division, a floor, a sort.  TEST INFRASTRUCTURE ONLY.

The rule, per sequence, with n the row count and voxel_size a finite float32 > 0:

    Voxel of a row.   For each component c, q_c = floorf(p_c / voxel_size): the correctly rounded float32 division (not
                      a multiplication by a reciprocal), then floorf.
    Griddable rows.   A row is griddable iff all three p_c are finite and -2^20 <= q_c < 2^20 for all c.  The test is
                      made on the float, before any conversion to an integer.
    Key.              key = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20): 63 bits.
    Score of a row.   The uint32 bit pattern of its confidence when confidence >= +0.0f holds in float32; otherwise 0.
                      So NaN and negative values score 0, and -0.0 scores as +0.0.  Bit patterns of non-negative floats
                      order like the floats, and +inf is the largest.  Without confidences every score is 0.
    Winner.           Among the griddable rows r < n of one voxel the winner has the largest score.  Ties go to the
                      lowest row.
    Keep mask.        keep[r] = 1 iff r < n and the row is not griddable or is its voxel's winner.  A non-griddable row
                      is always kept and never competes.  Rows in [n, n_bound) get 0 and never compete.
    Winner output.    winner[r] is the winner of r's voxel; r itself for a non-griddable row; -1 for r >= n.

No hash table here: the rows are sorted by (key, score descending, row ascending) and the first of each key wins."""
import numpy as np

LIM = np.float32(1 << 20)


def keys(points, voxel_size):
    """(key uint64 (rows,), griddable bool (rows,)); the key of a row that is not griddable is 0 and means nothing"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    vs = np.float32(voxel_size)
    assert np.isfinite(vs) and vs > 0
    with np.errstate(all="ignore"):
        q = np.floor(p / vs)                      # float32 / float32: IEEE, correctly rounded
        assert q.dtype == np.float32
        ok = (np.isfinite(p) & (q >= -LIM) & (q < LIM)).all(axis=1)
    qi = np.where(ok[:, None], q, 0).astype(np.int64) + (1 << 20)
    key = (qi[:, 0].astype(np.uint64) << np.uint64(42)) | (qi[:, 1].astype(np.uint64) << np.uint64(21)) | \
        qi[:, 2].astype(np.uint64)
    return np.where(ok, key, np.uint64(0)), ok


def scores(confidence, rows):
    """uint32 (rows,): the bit pattern of a confidence that is >= +0.0 (-0.0 as +0.0), else 0"""
    if confidence is None:
        return np.zeros(rows, np.uint32)
    c = np.ascontiguousarray(confidence, np.float32).reshape(-1)[:rows]
    with np.errstate(invalid="ignore"):
        ok = c >= np.float32(0.0)                 # NaN >= 0 is False
    return np.where(ok, c.view(np.uint32) & np.uint32(0x7FFFFFFF), np.uint32(0)).astype(np.uint32)


def voxel_keep(points, confidence, n, voxel_size):
    """One sequence: points (n_bound, 3) of which the first n are the map, confidence (n_bound,) / (n_bound, 1) or None.
    Returns (keep uint8 (n_bound,), winner int64 (n_bound,))."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n_bound, n = p.shape[0], int(n)
    assert 0 <= n <= n_bound
    keep = np.zeros(n_bound, np.uint8)
    winner = np.full(n_bound, -1, np.int64)
    key, ok = keys(p[:n], voxel_size)
    sc = scores(confidence, n)
    winner[:n] = np.arange(n)
    g = np.nonzero(ok)[0]
    if g.size:
        order = g[np.lexsort((g, -sc[g].astype(np.int64), key[g]))]   # by key, then score descending, then row
        first = np.ones(order.size, bool)
        first[1:] = key[order[1:]] != key[order[:-1]]
        lead = order[np.maximum.accumulate(np.where(first, np.arange(order.size), 0))]
        winner[order] = lead
    keep[:n] = winner[:n] == np.arange(n)
    return keep, winner


def thin_map(m, voxel_size):
    """The thinning of one step on an oracle map (oracle.slam's surfel store: points / normals / colors / ccounts), in
    place.  Returns the number of rows removed."""
    n = len(m)
    keep, _ = voxel_keep(m.points, m.ccounts, n, voxel_size)
    s = keep != 0
    m.points, m.normals, m.colors, m.ccounts = (np.ascontiguousarray(a[:n][s]) for a in
                                                (m.points, m.normals, m.colors, m.ccounts))
    return n - int(s.sum())
