"""The order contract of the projective ICP's ordered backward (gs_picp_bwd.hip, "ordered mode") as a plain loop, shared
by tests/test_picp_ordered_backward_cpu.py (CPU) and tests/test_hip_picp_ordered_backward.py (GPU).  No test lives here.

Given the record of every iteration -- keys (numiters, nslots): the slot's map row or NO_KEY; contrib (numiters, nslots,
6) float64: the slot's contribution to points_bar[row] (0:3) and to normals_bar[row] (3:6) -- the map gradients are:
  * acc[row] starts at +0.0;
  * the iterations are processed in launch order, numiters - 1 down to 0;
  * in an iteration a row's run sum starts at 0.0 and adds the contributions of its slots in ascending slot id, then
    acc[row] = acc[row] + run_sum;
  * a row that nobody touches ends as +0.0;
  * acc is rounded to float32 once at the end.
Every addition is one IEEE float64 addition (Python floats), none is vectorised or reordered."""
import numpy as np

NO_KEY = 0x7fffffff


def ordered_sum(keys, contrib, n_rows):
    """(points_bar, normals_bar), float32 (n_rows, 3) each, of the record by the contract above"""
    keys = np.asarray(keys)
    contrib = np.asarray(contrib, np.float64)
    assert keys.ndim == 2 and contrib.shape == keys.shape + (6,)
    acc = [[0.0] * 6 for _ in range(int(n_rows))]
    for it in range(keys.shape[0] - 1, -1, -1):
        run = {}                                   # row -> the run sum of this iteration
        for k in range(keys.shape[1]):             # ascending slot id
            row = int(keys[it, k])
            if row == NO_KEY:
                continue
            assert 0 <= row < n_rows, (it, k, row)
            s = run.get(row)
            if s is None:
                s = run[row] = [0.0] * 6
            for c in range(6):
                s[c] = s[c] + float(contrib[it, k, c])
        for row, s in run.items():                 # (the rows of an iteration are independent of each other)
            a = acc[row]
            for c in range(6):
                a[c] = a[c] + s[c]
    acc = np.array(acc, np.float64).reshape(int(n_rows), 6)
    return acc[:, :3].astype(np.float32), acc[:, 3:].astype(np.float32)
