"""GPU: both nearest-neighbour engines and the search inside the ICP solve against the ORACLE (oracle.knn1, a sequential
float32 scan on the CPU), never against each other, on the case families of tests/knn_cases.py: sizes on either side of
every launch constant, queries on and around the targets' bounding box, ties and near-ties, far-away and tiny clouds,
non-finite queries and targets, and more unresolved queries than one trip of the listed brute-force pass serves.
tests/test_knn_cases_cpu.py holds the oracle itself to float64 on the same cases.

Indices must be equal and squared distances equal bit for bit (no tolerance: every engine evaluates
fma(dz, dz, fma(dy, dy, dx * dx)) in float32 and orders candidates by (distance, index)).

Searches of the solve.  ops.icp_with_tape records, for every iteration k, the cloud at the start of the iteration and the
neighbour indices of its two searches.  tape_src[k] IS the query cloud of the first search: the half-iteration kernel (and
the brute-force path's search kernel) applies the pending transform on load and stores the transformed cloud into slot k
(icp_cloud() in csrc/gs_icp_loop.hip), and oracle/icp_backward.py reads it the same way (its rows are linearised at
tape["src"][k]).  So idx[k, 0] must equal oracle.knn1(tape_src[k], tgt) index by index.  The look-ahead indices idx[k, 1]
are NOT checked here: the look-ahead cloud is se3_exp(xi_k) applied to tape_src[k], and the HIP se3_exp is pinned to the
oracle's within 1e-7 only (tests/test_hip_parity.py::test_se3_exp_and_transform), not bit for bit, so that cloud cannot be
rebuilt exactly from the tape with the oracle's functions.  The knobs of the solve are read once per process, so the
solves run in child processes (one per lane count 2 / 4 / 8, one with the brute-force engine), each covering every cloud
in one launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as o
from tests import knn_cases as kc
from tests.test_hip_backward_kernels import read_tape
from tests.test_hip_engine_matrix import _child_env

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()   # (the shared cases are read-only arrays)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_oracle(tag, name, idx, d2):
    oi, od = kc.oracle_result(name)
    idx, d2 = host(idx), host(d2)
    bad = np.flatnonzero(idx != oi)
    assert bad.size == 0, "%s %s: %d of %d indices differ from the oracle, first at query %d: got %d (d2 %r), oracle %d " \
        "(d2 %r), query %r" % (tag, name, bad.size, len(oi), bad[0], idx[bad[0]], d2[bad[0]], oi[bad[0]], od[bad[0]],
                               kc.cases()[name][0][bad[0]])
    badd = np.flatnonzero(bits(d2) != bits(od))
    assert badd.size == 0, "%s %s: %d distances differ in bits, first at query %d: %r vs %r" % (
        tag, name, badd.size, badd[0], d2[badd[0]], od[badd[0]])


# ------------------------------------------------------------------------------------------------ the two engines
@pytest.mark.parametrize("name", kc.names())
def test_brute_force_engine_matches_oracle(ops, name):
    src, tgt, _ = kc.cases()[name]
    assert_oracle("knn1", name, *ops.knn1(dev(src), dev(tgt)))


@pytest.mark.parametrize("name", kc.names())
def test_grid_engine_matches_oracle(ops, name):
    src, tgt, _ = kc.cases()[name]
    assert_oracle("knn1_grid", name, *ops.knn1_grid(dev(src), dev(tgt)))


def test_listed_pass_loops_and_the_counter_is_rearmed(ops):
    """More unresolved queries than one trip of the listed brute-force pass serves (4 source tiles of 1 024), then a call on
    the same targets that leaves none: a counter left over from the call before would show."""
    src, tgt, _ = kc.cases()["far_all"]
    idx, d2, unres = ops.knn1_grid(dev(src), dev(tgt), return_unresolved=True)
    assert unres > kc.LISTED_TRIP, unres
    assert_oracle("knn1_grid", "far_all", idx, d2)
    src, tgt, _ = kc.cases()["far_then_near"]
    idx, d2, unres = ops.knn1_grid(dev(src), dev(tgt), return_unresolved=True)
    assert unres == 0, unres
    assert_oracle("knn1_grid", "far_then_near", idx, d2)


def test_call_sequence_reuses_the_workspace_in_both_phases(ops):
    """Growing and shrinking sizes back to back in one process; the sequence has an odd length and runs twice, so every
    case meets both phases of the grid query's ping-pong counter, and a workspace that has grown or is larger than needed."""
    for rep in range(2):
        for name in kc.CALL_SEQUENCE:
            src, tgt, _ = kc.cases()[name]
            idx, d2, unres = ops.knn1_grid(dev(src), dev(tgt), return_unresolved=True)
            assert_oracle("knn1_grid (call sequence, pass %d)" % rep, name, idx, d2)
            if name == "far_all":
                assert unres > kc.LISTED_TRIP, unres
            if name == "far_then_near":
                assert unres == 0, unres
            assert_oracle("knn1 (call sequence, pass %d)" % rep, name, *ops.knn1(dev(src), dev(tgt)))


# ------------------------------------------------------------------------------------------------ Gauss-Newton rows
def _same_rows(tag, got, ref):
    """bit for bit; where the oracle's value is NaN (a row of a non-finite query) any NaN will do"""
    got, ref = host(got) if torch.is_tensor(got) else got, np.asarray(ref)
    assert got.shape == ref.shape, tag
    if ref.dtype == np.float32:
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), tag
        assert np.array_equal(bits(got)[~nan], bits(ref)[~nan]), tag
    else:
        assert np.array_equal(got, ref), tag


@pytest.mark.parametrize("name", ["box_steps", "box_outside", "tie_midpoints", "tie_ulp_pairs", "nf_query_mixed"])
def test_gauss_newton_rows_match_oracle(ops, name):
    src, tgt, _ = kc.cases()[name]
    tn = kc.unit_normals(len(tgt), 11)
    _, od = kc.oracle_result(name)
    fin = od[np.isfinite(od)]
    exact = float(np.sort(fin)[len(fin) // 2])            # one query's exact d2: the comparison is strict, it must drop out
    assert (od == np.float32(exact)).any()
    for thr in (None, exact, -0.5, 0.0, float(np.nextafter(np.float32(exact), np.float32(np.inf)))):
        A, b, idx, keep = ops.gauss_newton_rows(dev(src), dev(tgt), dev(tn), thr)
        # (a negative threshold: no squared distance is below it, so like 0 it keeps no row -- ops._thresh; the oracle's
        # C entry reads a negative value as "no filter", hence its 0 stands for it)
        oA, ob, oidx, okeep = o.gauss_newton_rows(src, tgt, tn, thr if thr is None else max(thr, 0.0))
        tag = "%s dist_thresh=%r" % (name, thr)
        _same_rows(tag + " idx", idx, oidx)
        _same_rows(tag + " keep", keep, okeep)
        _same_rows(tag + " A", A, oA)
        _same_rows(tag + " b", b, ob)
        if thr == exact:
            assert not okeep[od == np.float32(exact)].any() and okeep.any()
        if thr is None:
            assert okeep.all()                             # no filter keeps every row, +inf distances included
        elif thr <= 0:
            assert not okeep.any() and not host(keep).any()


# ------------------------------------------------------------------------------------------------ searches of the solve
_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from gradslam_amd import ops
from tests import knn_cases as kc
out = sys.argv[1]
rec = {}
for n, (kind, ns, nt, mode) in enumerate(kc.solve_jobs(kc.SOLVE_GRID_SIZES + kc.SOLVE_BRUTE_SIZES)):
    src, tgt, tn, init = (torch.from_numpy(x).cuda() for x in kc.solve_case(kind, ns, nt))
    T, idx, tape, prm = ops.icp_with_tape(src, tgt, tn, init, numiters=kc.SOLVE_ITERS, mode=mode)
    torch.cuda.synchronize()
    rec["tape%%d" %% n] = tape.cpu().numpy()
    rec["T%%d" %% n] = T.cpu().numpy()
np.savez(out, **rec)
"""

CHILDREN = {
    "lanes2": {"GRADSLAM_HIP_ICP_LANES": "2"},
    "lanes4": {"GRADSLAM_HIP_ICP_LANES": "4"},
    "lanes8": {"GRADSLAM_HIP_ICP_LANES": "8"},
    "brute": {"GRADSLAM_HIP_KNN": "brute"},
}


@pytest.mark.parametrize("child", list(CHILDREN))
def test_every_search_of_the_solve_matches_oracle(tmp_path, child):
    """3 iterations in both LM modes from a non-identity init, on the grid side of the engine switch (n_src in {256, 257,
    351, 561}: a partial last unit of 96 points, partial lane groups; n_tgt in {2 048, 2 049, 3 000}) and on its
    brute-force side (255 x 3 000, 561 x 2 047): the first-half neighbour indices of every iteration are the oracle's
    for the cloud the tape recorded."""
    out = str(tmp_path / (child + ".npz"))
    subprocess.run([sys.executable, "-c", _CHILD % REPO, out], check=True, timeout=300, env=_child_env(CHILDREN[child]))
    r = np.load(out)
    jobs = kc.solve_jobs(kc.SOLVE_GRID_SIZES + kc.SOLVE_BRUTE_SIZES)
    far_seen = 0
    for n, (kind, ns, nt, mode) in enumerate(jobs):
        src, tgt, tn, init = kc.solve_case(kind, ns, nt)
        tp = read_tape(torch.from_numpy(r["tape%d" % n]), ns, {"numiters": kc.SOLVE_ITERS, "mode": mode}, init)
        assert tp["src"].shape == (kc.SOLVE_ITERS, ns, 3) and tp["idx"].shape == (kc.SOLVE_ITERS, 2, ns)
        assert np.isfinite(tp["src"]).all() and np.isfinite(r["T%d" % n]).all(), (child, kind, ns, nt, mode)
        # the first search's cloud: init applied to the source, the transform the oracle pins bit for bit
        assert np.array_equal(bits(tp["src"][0]), bits(o.transform_points(src, init))), (child, kind, ns, nt, mode)
        for k in range(kc.SOLVE_ITERS):
            oi, od = o.knn1(tp["src"][k], tgt)
            got = tp["idx"][k, 0]
            bad = np.flatnonzero(got != oi)
            assert bad.size == 0, "%s %s %dx%d mode %d iteration %d: %d indices differ from the oracle, first at point %d: " \
                "%d vs %d" % (child, kind, ns, nt, mode, k, bad.size, bad[0], got[bad[0]], oi[bad[0]])
            if kind == "border":
                far_seen += int((np.sqrt(od) > 0.5).sum())
            if k and mode == 1:   # (gradLM always steps; LM may reject a step and search the same cloud again)
                assert not np.array_equal(tp["src"][k], tp["src"][k - 1])
    assert far_seen > 30 * kc.SOLVE_ITERS          # the border clouds kept queries without a target within several cells
