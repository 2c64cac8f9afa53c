"""Point sets shared by tests/test_knn_cases_cpu.py (CPU) and tests/test_hip_knn_edges.py (GPU).  No test lives here.

Every family is a deterministic function of its seed and yields cases `(name, src, tgt, flags)`: float32 (n, 3) queries and
targets, and `flags["f64"]`, which says whether the float64 cross-check of the oracle applies (finite input whose squared
distances neither overflow nor underflow float32).  The families sit at the places where a nearest-neighbour engine goes
wrong without its suite noticing: sizes on either side of every launch constant, queries on and around the targets'
bounding box, ties and near-ties, clouds far from the origin or tiny, non-finite input, and more unresolved queries than
one trip of the listed brute-force pass serves.

`cases()` builds every case once per process; `oracle_result(name)` is the oracle's answer, computed once and shared
read-only."""
import functools

import numpy as np

F32 = np.float32

N_SRC_SIZES = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049)
N_TGT_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2047, 2048, 2049)
# every value of both lists at least once; the last rows sit on the four sides of the gs_knn_use_grid border
SIZE_PAIRS = ((1, 1), (7, 2), (8, 255), (9, 256), (31, 257), (32, 511), (33, 512), (255, 513), (256, 1025), (257, 2047),
              (1023, 2048), (1024, 2049), (1025, 1), (2049, 2049), (2049, 513), (33, 2049), (1, 2048),
              (255, 2048), (256, 2047), (256, 2048), (257, 2049))

N_BOX_TGT = 3000
FAR_N_SRC, FAR_N_TGT = 6000, 2500
FAR_SHIFT = (5.0, -3.0, 8.0)      # several box extents away from the surface: beyond the reach of the ring search
LISTED_TRIP = 4 * 1024             # queries that one trip of the listed brute-force pass serves (4 source tiles of 1 024)


def surface(rng, n, noise=0.0):
    """n points of a smooth sheet at depth ~2 (what an ICP target set looks like), optionally with Gaussian noise"""
    u, v = rng.random(n) * 2.4 - 1.2, rng.random(n) * 1.8 - 0.9
    z = 2.0 + 0.3 * np.sin(3 * u) * np.cos(2.5 * v)
    p = np.stack([u, v, z], -1)
    return (p + noise * rng.standard_normal(p.shape)).astype(F32)


def surface_normals(tgt):
    """unit normals of the sheet of surface() at the (x, y) of the targets"""
    u, v = tgt[:, 0].astype(np.float64), tgt[:, 1].astype(np.float64)
    n = np.stack([-0.9 * np.cos(3 * u) * np.cos(2.5 * v), 0.75 * np.sin(3 * u) * np.sin(2.5 * v), np.ones_like(u)], -1)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)


def unit_normals(n, seed):
    """n unit vectors that lean at most ~17 degrees away from +z (a well-conditioned point-to-plane system)"""
    v = np.random.default_rng(seed).standard_normal((n, 3)) * 0.15
    v[:, 2] = 1.0
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def f32_steps(x, n):
    """x moved n float32 values up (n > 0) or down (n < 0): np.nextafter applied |n| times"""
    i = np.asarray(x, F32).view(np.int32).astype(np.int64)
    k = np.where(i < 0, -(i & 0x7fffffff), i) + np.asarray(n, np.int64)   # ordered integer of the float
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(F32)


def d2_f32(q, t):
    """fma(dz, dz, fma(dy, dy, dx * dx)) in float32, row by row.  (The product of two float32 is exact in float64; the
    sum then rounds twice, which can differ from a true fma in rare half-way cases: the CPU suite holds every value this
    module relies on to the oracle's own distance.)"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    dx, dy, dz = ((q[..., k] - t[..., k]).astype(F32) for k in range(3))
    d = (dx * dx).astype(F32)
    d = (dy.astype(np.float64) * dy + d).astype(F32)
    return (dz.astype(np.float64) * dz + d).astype(F32)


# ------------------------------------------------------------------------------------------------ sizes
def size_cases(seed=101):
    for ns, nt in SIZE_PAIRS:
        rng = np.random.default_rng([seed, ns, nt])
        tgt = surface(rng, nt)
        yield "size_%dx%d" % (ns, nt), surface(rng, ns, noise=0.003), tgt, {"f64": True}


# ------------------------------------------------------------------------------------------------ box geometry
def box_targets(seed=202, n=N_BOX_TGT):
    return surface(np.random.default_rng(seed), n)


def box_queries(tgt, seed=203):
    """dict of query groups around the bounding box of tgt (every group float32 (m, 3))"""
    rng = np.random.default_rng(seed)
    lo, hi = tgt.min(0), tgt.max(0)
    ext = (hi - lo).astype(np.float64)
    mid = ((lo.astype(np.float64) + hi) / 2)
    pick = lambda b: np.array([(lo, mid, hi)[b[k]][k] for k in range(3)], np.float64)   # noqa: E731
    codes = [(a, b, c) for a in (0, 1, 2) for b in (0, 1, 2) for c in (0, 1, 2)]
    g = {}
    g["corners"] = np.stack([pick(b) for b in codes if b.count(1) == 0])
    g["edge_mids"] = np.stack([pick(b) for b in codes if b.count(1) == 1])
    g["face_mids"] = np.stack([pick(b) for b in codes if b.count(1) == 2])
    outside, steps_in, steps_out = [], [], []
    for axis in range(3):
        for side in (0, 1):
            face = (lo, hi)[side][axis]
            sign = -1.0 if side == 0 else 1.0
            for dist in (0.003, 0.05, 0.4, 1.0, 2.2, 3.6):     # in box extents of that axis
                p = lo + rng.random((6, 3)) * ext
                p[:, axis] = face + sign * dist * ext[axis]
                outside.append(p)
            # a few hundred float32 values inside and outside the face, at random places and under the extreme target
            at = np.concatenate([lo + rng.random((5, 3)) * ext, tgt[[tgt[:, axis].argmin() if side == 0 else
                                                                        tgt[:, axis].argmax()]].astype(np.float64)])
            for n in (1, 2, 17, 100, 300, 700):
                pin, pout = at.astype(F32), at.astype(F32)
                pin[:, axis] = f32_steps(np.full(len(at), face, F32), int(-sign * n))
                pout[:, axis] = f32_steps(np.full(len(at), face, F32), int(sign * n))
                steps_in.append(pin)
                steps_out.append(pout)
    g["outside_faces"] = np.concatenate(outside)
    g["steps_inside"] = np.concatenate(steps_in)
    g["steps_outside"] = np.concatenate(steps_out)
    diag = []
    for b in codes:
        if b.count(1) == 0:
            d = np.array([(-1.0, 0.0, 1.0)[c] for c in b])
            for dist in (0.01, 0.3, 1.5, 3.6):
                diag.append(pick(b) + d * dist * ext * (0.5 + rng.random(3)))
    g["outside_diagonal"] = np.stack(diag)
    return {k: np.ascontiguousarray(v, dtype=F32) for k, v in g.items()}


def box_cases():
    tgt = box_targets()
    g = box_queries(tgt)
    yield "box_on", np.concatenate([g["corners"], g["edge_mids"], g["face_mids"]]), tgt, {"f64": True}
    yield "box_outside", np.concatenate([g["outside_faces"], g["outside_diagonal"]]), tgt, {"f64": True}
    yield "box_steps", np.concatenate([g["steps_inside"], g["steps_outside"]]), tgt, {"f64": True}


# ------------------------------------------------------------------------------------------------ near-ties
TIE_LATTICE = (14, 14, 12)
TIE_PAIRS = 64
TIE_DUPS = 32


def _lattice(shape, seed):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3).astype(F32)
    return g[np.random.default_rng(seed).permutation(len(g))]


def lattice_queries(shape, seed, n=None):
    """cell mid-points of the lattice (8 equidistant targets each) and the mid-points moved one float32 value along +-
    each axis (4 equidistant targets, the other 4 a few float32 values of the distance behind -- or still 8 where the
    step is lost in the distance's rounding); n: that many of them, mixed"""
    mids = np.stack(np.meshgrid(*[np.arange(s - 1) for s in shape], indexing="ij"), -1).reshape(-1, 3).astype(F32) + F32(0.5)
    rng = np.random.default_rng(seed)
    mids = mids[rng.permutation(len(mids))][:640]
    out = [mids]
    for axis in range(3):
        for n_step in (1, -1):
            m = mids.copy()
            m[:, axis] = f32_steps(m[:, axis], n_step)
            out.append(m)
    q = np.concatenate(out)
    if n is not None:
        q = q[rng.permutation(len(q))[:n]]
    return np.ascontiguousarray(q)


def ulp_pairs(n, seed, z=15.0):
    """(q, a, b): n isolated triples with d2(q, b) exactly one float32 value BELOW d2(q, a); a, b ~0.35 from q on opposite
    sides, the triples 1.6 apart on the plane z"""
    rng = np.random.default_rng(seed)
    q = np.stack([0.8 + 1.6 * (np.arange(n) % 8), 0.8 + 1.6 * (np.arange(n) // 8), np.full(n, z)], -1).astype(F32)
    q += (rng.random((n, 3)) * 0.01).astype(F32)
    a, b = np.zeros_like(q), np.zeros_like(q)
    for i in range(n):
        while True:
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            r = 0.3 + 0.1 * rng.random()
            ai = (q[i] + r * d).astype(F32)
            cand = (q[i][None] - (r * (1.0 - rng.random((256, 1)) * 4e-7)) * d[None]).astype(F32)
            gap = d2_f32(q[i], ai).view(np.int32).astype(np.int64) - d2_f32(q[i][None], cand).view(np.int32)
            hit = np.flatnonzero(gap == 1)
            if len(hit):
                a[i], b[i] = ai, cand[hit[0]]
                break
    return q, a, b


def tie_layout():
    """index ranges of the blocks of the near-tie target set: [a of the pairs | low duplicates | lattice | high
    duplicates | b of the pairs]"""
    nl = int(np.prod(TIE_LATTICE))
    edges = np.cumsum([0, TIE_PAIRS, TIE_DUPS, nl, TIE_DUPS, TIE_PAIRS])
    return dict(zip(("a", "dup_lo", "lattice", "dup_hi", "b"), zip(edges[:-1], edges[1:])))


@functools.lru_cache(maxsize=None)
def tie_targets(seed=303):
    lat = _lattice(TIE_LATTICE, seed)
    q, a, b = ulp_pairs(TIE_PAIRS, seed + 1)
    dup_lo, dup_hi = lat[100:100 + TIE_DUPS], lat[900:900 + TIE_DUPS]
    return np.ascontiguousarray(np.concatenate([a, dup_lo, lat, dup_hi, b])), q, dup_lo, dup_hi


def tie_cases(seed=303):
    tgt, pq, dup_lo, dup_hi = tie_targets(seed)
    yield "tie_midpoints", lattice_queries(TIE_LATTICE, seed + 2), tgt, {"f64": True}
    yield "tie_ulp_pairs", pq, tgt, {"f64": True}
    rng = np.random.default_rng(seed + 3)
    dups = np.concatenate([dup_lo, dup_hi])
    near = dups + (rng.standard_normal(dups.shape) * 0.05).astype(F32)
    yield "tie_duplicates", np.ascontiguousarray(np.concatenate([dups, near])), tgt, {"f64": True}


# ------------------------------------------------------------------------------------------------ scale
def scale_cases(seed=404):
    rng = np.random.default_rng(seed)
    tgt, src = surface(rng, 2600), surface(rng, 700, noise=0.003)
    yield "scale_offset_1e4", src + F32(1e4), tgt + F32(1e4), {"f64": True}
    yield "scale_1e-4", src * F32(1e-4), tgt * F32(1e-4), {"f64": True}
    yield "scale_1e-7", src * F32(1e-7), tgt * F32(1e-7), {"f64": True}
    # float32 denormals (multiples of 2**-149 below 2**-126) next to a few rows at 1e-3; squared distances underflow
    tiny = F32(2.0 ** -149)
    dt = (rng.integers(-4000000, 4000000, (2200, 3)).astype(F32) * tiny).astype(F32)
    ds = (rng.integers(-4000000, 4000000, (300, 3)).astype(F32) * tiny).astype(F32)
    t = np.concatenate([dt[:1100], tgt[:200] * F32(1e-3), dt[1100:]])
    s = np.concatenate([ds, src[:300] * F32(1e-3)])
    yield "scale_denormal", np.ascontiguousarray(s), np.ascontiguousarray(t), {"f64": False}


# ------------------------------------------------------------------------------------------------ non-finite input
def odd_queries(base):
    """base (finite queries) followed by its rows made non-finite in every way the contract names; returns (queries,
    kinds): kinds[i] in {"finite", "nan", "inf", "far"}"""
    m = len(base)
    nan1, nan3, inf, far = base.copy(), base.copy(), base.copy(), base.copy()
    nan1[np.arange(m), np.arange(m) % 3] = np.nan
    nan3[:] = np.nan
    inf[np.arange(m), np.arange(m) % 3] = np.where(np.arange(m) % 2 == 0, np.inf, -np.inf)
    inf[::5] = np.inf
    far[np.arange(m), np.arange(m) % 3] = np.where(np.arange(m) % 2 == 0, 1e20, -1e20)
    far[::5] = 1e20
    q = np.concatenate([base, nan1, nan3, inf, far]).astype(F32)
    kinds = np.repeat(np.array(["finite", "nan", "nan", "inf", "far"]), m)
    return np.ascontiguousarray(q), kinds


def nonfinite_cases(seed=505):
    rng = np.random.default_rng(seed)
    tgt, base = surface(rng, 3000), surface(rng, 150, noise=0.003)
    q, kinds = odd_queries(base)
    off = {"f64": False}
    yield "nf_query_nan_one", q[150:300], tgt, off
    yield "nf_query_nan_all", q[300:450], tgt, off
    yield "nf_query_inf", q[450:600], tgt, off
    yield "nf_query_1e20", q[600:750], tgt, off
    yield "nf_query_mixed", q, tgt, off
    yield "nf_target_all_nan", q, np.full((2100, 3), np.nan, F32), off
    for nt, row in ((2100, 1234), (2100, 0), (300, 299), (2, 1)):
        one = np.full((nt, 3), np.nan, F32)
        one[row] = tgt[row]
        yield "nf_target_one_finite_%d_of_%d" % (row, nt), q, one, off
    for first, last in ((np.nan, np.inf), (np.inf, np.nan), (-np.inf, np.inf)):
        t = tgt.copy()
        t[0], t[-1] = first, last
        t[1, 1], t[-2, 2] = np.nan, np.inf        # rows that are non-finite in one component only
        yield "nf_target_ends_%s_%s" % (first, last), q, t, off
    # the same ends on a cloud that collapses into a grid of 2 x 2 x 2 cells
    t = tgt * F32(1e-7)
    t[0], t[-1] = np.nan, np.inf
    yield "nf_target_ends_tiny", np.ascontiguousarray(np.concatenate([q[:150] * F32(1e-7), q[150:]])), t, off


# ------------------------------------------------------------------------------------------------ many unresolved
def far_targets(seed=606):
    return surface(np.random.default_rng(seed), FAR_N_TGT)


def far_cases(seed=606):
    tgt = far_targets(seed)
    rng = np.random.default_rng(seed + 1)
    yield "far_all", surface(rng, FAR_N_SRC) + np.array(FAR_SHIFT, F32), tgt, {"f64": True}
    yield "far_then_near", surface(rng, FAR_N_SRC, noise=0.002), tgt, {"f64": True}


# ------------------------------------------------------------------------------------------------ registry
FAMILIES = (size_cases, box_cases, tie_cases, scale_cases, nonfinite_cases, far_cases)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (src, tgt, flags)} of every family, built once; the arrays are read-only"""
    out = {}
    for fam in FAMILIES:
        for name, src, tgt, flags in fam():
            src, tgt = np.ascontiguousarray(src, dtype=F32), np.ascontiguousarray(tgt, dtype=F32)
            assert name not in out and src.ndim == 2 and src.shape[1] == 3 and tgt.ndim == 2 and tgt.shape[1] == 3
            src.setflags(write=False)
            tgt.setflags(write=False)
            out[name] = (src, tgt, dict(flags))
    return out


def names(f64=None):
    return [n for n, c in cases().items() if f64 is None or c[2]["f64"] == f64]


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """(idx int64, d2 float32) of oracle.knn1 for the case, computed once, read-only"""
    from oracle import oracle as o
    src, tgt, _ = cases()[name]
    idx, d2 = o.knn1(src, tgt)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


# back-to-back calls of one process: sizes grow and shrink (the workspace grows, then is larger than needed), 7 calls, so
# that running the sequence twice shows every case both phases of the grid query's ping-pong counter
CALL_SEQUENCE = ("size_1x1", "size_2049x2049", "box_outside", "size_7x2", "far_all", "far_then_near", "size_33x512")


# ------------------------------------------------------------------------------------------------ searches of the solve
SOLVE_SETS = ("box", "tie", "border")
SOLVE_GRID_SIZES = ((256, 2048), (257, 2049), (351, 3000), (561, 2048), (561, 3000))
SOLVE_BRUTE_SIZES = ((255, 3000), (561, 2047))
SOLVE_ITERS = 3


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ \
        np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@functools.lru_cache(maxsize=None)
def solve_case(kind, n_src, n_tgt, seed=707):
    """(src, tgt, tgt_normals, init) of one ICP solve whose FIRST search sees the query set `kind` (up to the rounding of
    init applied to src); the later searches see what the solve makes of it.
      box:    the box-geometry queries (on, around and float32 steps off the targets' bounding box)
      tie:    lattice mid-points against the permuted integer lattice (+ duplicates with higher indices); init is a pure
              translation by binary fractions, so the first search sees the mid-points exactly
      border: a noisy copy of the surface of which one side looks past the targets (no target within several cells)"""
    rng = np.random.default_rng([seed, n_src, n_tgt, SOLVE_SETS.index(kind)])
    if kind == "tie":
        shape = (16, 16, 8)
        lat = _lattice(shape, seed)
        tgt = np.concatenate([lat, lat[:max(n_tgt - len(lat), 0)]])[:n_tgt]   # (short of the lattice: its last rows are missing)
        tn = unit_normals(n_tgt, seed + 1)
        shift = np.array([0.5, -0.25, 0.125])
        q = lattice_queries(shape, seed + 2, n_src)
        init = np.eye(4)
        init[:3, 3] = shift
        src = (q.astype(np.float64) - shift).astype(F32)
    else:
        tgt = surface(rng, n_tgt)
        tn = surface_normals(tgt)
        if kind == "box":
            g = box_queries(tgt, seed + 3)
            q = np.concatenate(list(g.values()))
            q = q[rng.permutation(len(q))[:n_src]]
        else:
            q = surface(rng, n_src, noise=0.003)
            side = q[:, 0] > 0.7
            q[side, 0] += F32(1.1)      # past the edge of the targets: their neighbours are several cells away
            q[side, 2] += F32(0.6)
        assert len(q) == n_src
        init = _rigid(0.02, -0.015, 0.03, [0.01, -0.02, 0.015])
        inv = np.linalg.inv(init)
        src = (q.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    out = tuple(np.ascontiguousarray(x, dtype=F32) for x in (src, tgt, tn, init))
    for x in out:
        x.setflags(write=False)
    return out


def solve_jobs(sizes):
    """(kind, n_src, n_tgt, mode) of every solve of a child process"""
    return [(k, ns, nt, mode) for k in SOLVE_SETS for ns, nt in sizes for mode in (0, 1)]
