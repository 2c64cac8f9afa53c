"""NumPy restatement of the map prune (gs_prune.hip -> gs_prune_map_dc_f32 -> ops.prune_map_batch ->
Pointclouds.prune_): a boolean rule, `arr[:n][survive]`, and a cumulative sum for the epoch marks.

Row r of a map of n rows survives iff

    (keep is None or keep[r] != 0) and
    (min_confidence is None or r >= young_from or ccounts[r] >= min_confidence)

with a float32 comparison (a NaN confidence fails it, a confidence bit-equal to the threshold passes).  young_from is
marks[young_mark] as it stands BEFORE the prune; young_mark = -1 means that every row is old enough.  After the prune mark m
is the number of survivors among the rows < min(m, n).  The operation moves bits: nothing here rounds."""
import numpy as np


def survivors(n, ccounts=None, min_confidence=None, keep=None, marks=(), young_mark=-1):
    """(n,) bool: which of the first n rows survive."""
    n = int(n)
    s = np.ones(n, dtype=bool)
    if keep is not None:
        s &= np.asarray(keep).reshape(-1)[:n] != 0
    if min_confidence is not None:
        young_from = n if young_mark < 0 else min(int(marks[young_mark]), n)
        cc = np.asarray(ccounts, dtype=np.float32).reshape(-1)[:n]
        with np.errstate(invalid="ignore"):
            passes = cc >= np.float32(min_confidence)          # NaN >= x is False
        s &= (np.arange(n) >= young_from) | passes
    return s


def remap_marks(survive, marks):
    n = survive.shape[0]
    before = np.concatenate([[0], np.cumsum(survive, dtype=np.int64)])   # before[r] = survivors among rows < r
    return [int(before[min(int(m), n)]) for m in marks]


def prune(points, normals, colors, features, n, min_confidence=None, keep=None, marks=(), young_mark=-1):
    """One sequence.  points / normals / colors (rows, 3), features (rows, F), rows >= n; normals / colors / features may be
    None.  The confidence is feature channel 0.  Returns (points, normals, colors, features, new_n, removed, new_marks),
    the arrays holding exactly new_n rows."""
    n = int(n)
    cc = None
    if min_confidence is not None:
        assert features is not None and features.shape[1] == 1, "the confidence rule needs one feature channel"
        cc = features[:, 0]
    s = survivors(n, cc, min_confidence, keep, marks, young_mark)
    out = tuple(None if a is None else np.ascontiguousarray(a[:n][s]) for a in (points, normals, colors, features))
    kept = int(s.sum())
    return out + (kept, n - kept, remap_marks(s, marks))
