"""CPU: the oracle's nearest-neighbour search (oracle.knn1, a sequential float32 scan) on the case families of
tests/knn_cases.py -- the reference tests/test_hip_knn_edges.py holds both HIP engines to.

  * against float64: the index the oracle returns is a float64 nearest neighbour up to the rounding of the two float32
    distances it compared.  With u = 2**-24 each distance fma(dz, dz, fma(dy, dy, dx * dx)) carries at most ~6u of relative
    error (one rounding per difference, entering squared; one per product / fma), so the order of two distances can only
    flip inside a ratio of 1 + 12u; 16u = 2**-20 rounds that up.  No query is excluded.
  * its semantics on non-finite input, as literal expectations (what the HIP engines must reproduce);
  * that every family is what its name says."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import knn_cases as kc

F64_SLACK = 2.0 ** -20


@pytest.mark.parametrize("name", kc.names(f64=True))
def test_oracle_index_is_a_float64_nearest_neighbour(name):
    src, tgt, _ = kc.cases()[name]
    idx, d2 = kc.oracle_result(name)
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    dmin = np.empty(len(s))
    dgot = np.empty(len(s))
    for a in range(0, len(s), 512):
        d = ((s[a:a + 512, None, :] - t[None]) ** 2).sum(-1)
        dmin[a:a + 512] = d.min(1)
        dgot[a:a + 512] = d[np.arange(d.shape[0]), idx[a:a + 512]]
    excess = dgot - dmin * (1.0 + F64_SLACK)
    assert (excess <= 0).all(), (name, int((excess > 0).sum()), float((dgot / np.maximum(dmin, 1e-300)).max()))
    # the distance it reports is that pair's distance, within the ~6u of its float32 evaluation
    np.testing.assert_allclose(d2, dgot, rtol=8 * 2.0 ** -24, atol=0)


def test_oracle_breaks_ties_towards_the_lowest_index():
    src, tgt, _ = kc.cases()["tie_midpoints"]
    idx, d2 = kc.oracle_result("tie_midpoints")
    d = np.stack([kc.d2_f32(src, np.broadcast_to(t, src.shape)) for t in tgt], 1)     # the float32 distances themselves
    assert np.array_equal(d2, d.min(1))
    assert np.array_equal(idx, d.argmin(1))          # argmin: the first of equal minima


# ------------------------------------------------------------------------------------------------ non-finite input
def _kinds(n_base=150):
    return np.repeat(np.array(["finite", "nan", "nan", "inf", "far"]), n_base)


@pytest.mark.parametrize("name", ["nf_query_nan_one", "nf_query_nan_all", "nf_query_inf", "nf_query_1e20"])
def test_oracle_gives_index_0_and_inf_to_a_query_without_a_finite_distance(name):
    idx, d2 = kc.oracle_result(name)
    assert len(idx) == 150 and (idx == 0).all() and np.isposinf(d2).all()


def test_oracle_on_mixed_queries():
    idx, d2 = kc.oracle_result("nf_query_mixed")
    fin = _kinds() == "finite"
    assert np.isfinite(d2[fin]).all() and (idx[~fin] == 0).all() and np.isposinf(d2[~fin]).all()


def test_oracle_on_all_nan_targets():
    idx, d2 = kc.oracle_result("nf_target_all_nan")
    assert (idx == 0).all() and np.isposinf(d2).all()


@pytest.mark.parametrize("row,nt", [(1234, 2100), (0, 2100), (299, 300), (1, 2)])
def test_oracle_on_one_finite_target(row, nt):
    name = "nf_target_one_finite_%d_of_%d" % (row, nt)
    src, tgt, _ = kc.cases()[name]
    assert tgt.shape == (nt, 3) and np.isfinite(tgt).all(1).sum() == 1 and np.isfinite(tgt[row]).all()
    idx, d2 = kc.oracle_result(name)
    fin = _kinds() == "finite"
    assert (idx[fin] == row).all() and np.isfinite(d2[fin]).all()
    assert (idx[~fin] == 0).all() and np.isposinf(d2[~fin]).all()      # NaN, +-inf and 1e20 queries alike


@pytest.mark.parametrize("name", ["nf_target_ends_nan_inf", "nf_target_ends_inf_nan", "nf_target_ends_-inf_inf",
                                  "nf_target_ends_tiny"])
def test_oracle_ignores_non_finite_rows_at_either_end(name):
    src, tgt, _ = kc.cases()[name]
    assert not np.isfinite(tgt[0]).any() and not np.isfinite(tgt[-1]).any()
    idx, d2 = kc.oracle_result(name)
    fin = _kinds() == "finite"
    assert np.isfinite(tgt[idx[fin]]).all() and np.isfinite(d2[fin]).all()
    assert (idx[~fin] == 0).all() and np.isposinf(d2[~fin]).all()
    # the same answer as on the finite rows alone
    rows = np.flatnonzero(np.isfinite(tgt).all(1))
    ri, rd = o.knn1(src[fin], tgt[rows])
    assert np.array_equal(rows[ri], idx[fin]) and np.array_equal(rd, d2[fin])


def test_oracle_on_denormal_coordinates():
    src, tgt, _ = kc.cases()["scale_denormal"]
    tiny = np.float32(2.0 ** -126)
    assert (np.abs(tgt[:1100]) < tiny).all() and (np.abs(src[:300]) < tiny).all() and (tgt[:1100] != 0).any()
    idx, d2 = kc.oracle_result("scale_denormal")
    assert (idx[:300] == 0).all() and (d2[:300] == 0).all()       # every such distance underflows: the first target wins
    assert ((idx[300:] >= 1100) & (idx[300:] < 1300)).all() and (d2[300:] > 0).all()


# ------------------------------------------------------------------------------------------------ family integrity
def test_sizes_are_as_listed():
    c = kc.cases()
    got = {(c[n][0].shape[0], c[n][1].shape[0]) for n in c if n.startswith("size_")}
    assert got == set(kc.SIZE_PAIRS) and len(kc.SIZE_PAIRS) <= 24
    assert {p[0] for p in kc.SIZE_PAIRS} == set(kc.N_SRC_SIZES) and {p[1] for p in kc.SIZE_PAIRS} == set(kc.N_TGT_SIZES)
    assert kc.N_SRC_SIZES == (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049)
    assert kc.N_TGT_SIZES == (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2047, 2048, 2049)
    assert max(s.shape[0] * t.shape[0] for s, t, _ in c.values()) <= 6000 * 3000
    for name in kc.CALL_SEQUENCE:
        assert name in c
    assert len(kc.CALL_SEQUENCE) % 2 == 1


def test_box_families_lie_where_they_say():
    tgt = kc.box_targets()
    assert tgt.shape == (kc.N_BOX_TGT, 3)
    lo, hi = tgt.min(0), tgt.max(0)
    g = kc.box_queries(tgt)
    on = lambda q: (q == lo) | (q == hi)   # noqa: E731
    assert g["corners"].shape == (8, 3) and on(g["corners"]).all()
    assert len(np.unique(g["corners"], axis=0)) == 8
    assert g["edge_mids"].shape == (12, 3) and (on(g["edge_mids"]).sum(1) == 2).all()
    assert g["face_mids"].shape == (6, 3) and (on(g["face_mids"]).sum(1) == 1).all()
    out = lambda q: (q < lo) | (q > hi)   # noqa: E731
    assert (out(g["outside_faces"]).sum(1) == 1).all()
    for axis in range(3):       # each of the six sides, up to 3.6 extents away
        for far in (lo[axis] - g["outside_faces"][:, axis], g["outside_faces"][:, axis] - hi[axis]):
            assert 3.5 < far.max() / (hi[axis] - lo[axis]) < 3.7
    assert (out(g["outside_diagonal"]).sum(1) == 3).all() and len(g["outside_diagonal"]) == 32
    assert (out(g["steps_outside"]).sum(1) == 1).all() and not out(g["steps_inside"]).any()
    for q in (g["steps_inside"], g["steps_outside"]):
        # within a few hundred float32 values of a face, on every one of the six
        near = np.stack([np.minimum(np.abs(q[:, k].view(np.int32).astype(np.int64) - lo[k].view(np.int32)),
                                    np.abs(q[:, k].view(np.int32).astype(np.int64) - hi[k].view(np.int32))) for k in range(3)], 1)
        assert (near.min(1) >= 1).all() and (near.min(1) <= 700).all()
        hit = {(k, side) for k in range(3) for side in (0, 1)
               if (np.abs(q[:, k].view(np.int32).astype(np.int64) - (lo, hi)[side][k].view(np.int32)) <= 700).any()}
        assert len(hit) == 6


def test_f32_steps_is_repeated_nextafter():
    x = np.array([1.0, -1.0, 0.0, 2.0 ** -126, -2.0 ** -149, 3.5], np.float32)
    up, down = x.copy(), x.copy()
    for _ in range(5):
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
    assert np.array_equal(kc.f32_steps(x, 5), up) and np.array_equal(kc.f32_steps(x, -5), down)


def test_near_tie_families_contain_their_ties():
    tgt, pq, dup_lo, dup_hi = kc.tie_targets()
    lay = kc.tie_layout()
    assert len(tgt) == lay["b"][1] and np.array_equal(tgt[slice(*lay["dup_lo"])], dup_lo)
    lat = tgt[slice(*lay["lattice"])]
    assert np.array_equal(np.sort(lat.view("f4,f4,f4").ravel()),
                          np.sort(kc._lattice(kc.TIE_LATTICE, 0).view("f4,f4,f4").ravel()))   # the whole lattice...
    assert not np.array_equal(lat, lat[np.lexsort(lat.T[::-1])])                            # ...in a shuffled order
    one = lambda q, t: o.knn1(q, t[None])[1]       # the oracle's own distance of a pair   # noqa: E731
    # pairs: b (the higher index) is nearer than a by exactly one float32 value, and the oracle picks it
    a, b = tgt[slice(*lay["a"])], tgt[slice(*lay["b"])]
    da = np.array([one(pq[i:i + 1], a[i])[0] for i in range(len(pq))], np.float32)
    db = np.array([one(pq[i:i + 1], b[i])[0] for i in range(len(pq))], np.float32)
    assert np.array_equal(da.view(np.int32) - db.view(np.int32), np.ones(len(pq), np.int32))
    idx, d2 = kc.oracle_result("tie_ulp_pairs")
    assert np.array_equal(idx, np.arange(*lay["b"])) and np.array_equal(d2, db)
    # mid-points: 8 targets at exactly the minimum; moved one float32 value along an axis: 4 (where the step is lost in the
    # rounding of the distance: still 8), the other 4 a few float32 values of the distance behind (a step of one ulp of
    # a coordinate up to 13.5 is 16 ulps of the distance 0.75 at the most)
    src = kc.cases()["tie_midpoints"][0]
    idx, d2 = kc.oracle_result("tie_midpoints")
    d = np.stack([kc.d2_f32(src, np.broadcast_to(t, src.shape)) for t in lat], 1)
    at_min = (d == d2[:, None]).sum(1)
    four = np.flatnonzero(at_min == 4)
    assert (at_min[:640] == 8).all() and ((at_min == 4) | (at_min == 8)).all() and (four >= 640).all() and len(four) > 3000
    gap = np.partition(d.view(np.int32), 4, axis=1)[:, 4] - d2.view(np.int32)
    assert (gap[four] >= 1).all() and (gap[four] <= 32).all()
    # ...and the winner is the lowest INDEX among them (a low duplicate where one takes part), not the first in lattice order
    tied = d == d2[:, None]
    first = lay["lattice"][0] + tied.argmax(1)
    plain = idx >= lay["lattice"][0]
    assert np.array_equal(idx[plain], first[plain]) and plain.sum() > 4000 and (~plain).sum() > 0
    assert (idx[~plain] >= lay["dup_lo"][0]).all() and len(np.unique(idx)) > 300
    order = np.lexsort(lat.T[::-1])                       # lattice order: x fastest ... the order a plain meshgrid would give
    rank = np.empty(len(lat), np.int64)
    rank[order] = np.arange(len(lat))
    lowest_rank = np.where(tied, rank[None], len(lat)).argmin(1)
    assert (lowest_rank != tied.argmax(1)).sum() > 2000    # the permutation decides most winners
    # duplicates: exact hits; the copy at the low end wins over the lattice point, the lattice point over the copy at the
    # high end
    idx, d2 = kc.oracle_result("tie_duplicates")
    n = kc.TIE_DUPS
    assert (d2[:2 * n] == 0).all()
    assert np.array_equal(idx[:n], np.arange(*lay["dup_lo"]))
    assert ((idx[n:2 * n] >= lay["lattice"][0]) & (idx[n:2 * n] < lay["lattice"][1])).all()
    assert np.array_equal(tgt[idx[n:2 * n]], dup_hi)


def test_scale_families():
    c = kc.cases()
    assert c["scale_offset_1e4"][1].min() > 9990 and np.ptp(c["scale_offset_1e4"][1], axis=0).max() < 3
    assert np.abs(c["scale_1e-4"][1]).max() < 3e-4
    t = c["scale_1e-7"][1]
    assert np.abs(t).max() < 3e-7 and (np.ptp(t, axis=0) < 1e-6).all()       # below the 1e-6 floor of the cell edge
    for name in ("scale_offset_1e4", "scale_1e-4", "scale_1e-7"):
        assert len(np.unique(kc.oracle_result(name)[0])) > 300                # still distinct neighbours


def test_far_family_is_out_of_reach():
    src, tgt, _ = kc.cases()["far_all"]
    assert src.shape == (kc.FAR_N_SRC, 3) and tgt.shape == (kc.FAR_N_TGT, 3) and kc.FAR_N_SRC > kc.LISTED_TRIP
    _, d2 = kc.oracle_result("far_all")
    assert np.sqrt(d2.min()) > 2 * np.ptp(tgt, axis=0).max()                # farther than twice the largest box extent
    _, d2 = kc.oracle_result("far_then_near")
    assert np.sqrt(d2.max()) < 0.1


def test_solve_cases_are_well_formed():
    for kind, ns, nt, _ in kc.solve_jobs(kc.SOLVE_GRID_SIZES + kc.SOLVE_BRUTE_SIZES):
        src, tgt, tn, init = kc.solve_case(kind, ns, nt)
        assert src.shape == (ns, 3) and tgt.shape == tn.shape == (nt, 3) and init.shape == (4, 4)
        assert np.isfinite(src).all() and not np.array_equal(init, np.eye(4, dtype=np.float32))
        np.testing.assert_allclose(np.linalg.norm(tn, axis=1), 1.0, atol=1e-6)
        np.testing.assert_allclose(init[:3, :3] @ init[:3, :3].T, np.eye(3), atol=1e-6)
    assert {s[0] for s in kc.SOLVE_GRID_SIZES} == {256, 257, 351, 561}
    assert {s[1] for s in kc.SOLVE_GRID_SIZES} == {2048, 2049, 3000}
    assert all(ns >= 256 and nt >= 2048 for ns, nt in kc.SOLVE_GRID_SIZES)
    assert set(kc.SOLVE_BRUTE_SIZES) == {(255, 3000), (561, 2047)}
    # the tie set: init applied to src gives the lattice mid-points back exactly
    src, tgt, _, init = kc.solve_case("tie", 561, 2049)
    q = o.transform_points(src, init)
    frac = q - np.floor(q)
    assert (np.abs(frac - 0.5) < 1e-6).all() and ((frac == 0.5).all(1)).sum() > 50
    # the border set: part of the queries has no target within several cell edges
    src, tgt, _, init = kc.solve_case("border", 561, 3000)
    _, d2 = o.knn1(o.transform_points(src, init), tgt)
    assert (np.sqrt(d2) > 0.5).sum() > 30 and (np.sqrt(d2) < 0.02).sum() > 200
