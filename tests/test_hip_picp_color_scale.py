"""GPU tests of the joint projective ICP's colour Huber threshold from the colour residuals' median (the joint residual
pass and the B x thresholds select of gs_picp_scale.hip in front of the robust kernel of gs_picp_color.hip: the
*_color_joint_scaled_* entry points -> ops.projective_icp_color*(color_huber_k=...) -> ProjectiveICPOdometryProvider ->
ICPSLAM / PointFusion(odom="projicp", color_weight=..., color_huber_k=...)).

The selection is exact (integer counting over the bit patterns of |r|) and every other operation is restated in the same
order by tests/picp_color_scale_ref.py, so every comparison -- thresholds, weights, sums, poses, traces -- is for EQUAL
BITS: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from tests import picp_color_ref as pcr
from tests import picp_color_scale_ref as csr
from tests import picp_robust_ref as rr
from tests import picp_scale_ref as sr
from tests.test_hip_picp import bits, dev, host
from tests.test_hip_picp_color import batch_call, color_edge_fixture, solve_hip, three_sequences
from tests.test_hip_picp_robust import geo, hand_written_loop, make_slam, same_run, same_solve, textured_frames
from tests.test_hip_picp_scale import MULTISETS, _multiset

pytestmark = pytest.mark.gpu

F = np.float32
K = csr.K_HUBER
WEIGHT = 0.2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gs():
    assert torch.cuda.is_available()
    import gradslam_amd
    return gradslam_amd


def colour(fx):
    return [dev(fx["color"]), dev(fx["model"])]


def same_rows(got, want, what=""):
    """(ProjectiveColorRows, weight, colour weight, delta, cdelta) of the device against the restated Rows, bit for bit"""
    rows_, weight, cweight, delta, cdelta = got
    torch.cuda.synchronize()
    assert bits(host(cdelta)[0]) == bits(want.cdelta), (what, host(cdelta), want.cdelta)
    assert bits(host(delta)[0]) == bits(want.delta), (what, host(delta), want.delta)
    assert np.array_equal(host(rows_.code), want.code) and np.array_equal(host(rows_.row), want.row), what
    assert np.array_equal(host(rows_.colored) == 1, want.colored), what
    for name in ("a", "b", "ac", "bc", "sums"):
        assert np.array_equal(bits(host(getattr(rows_, name))), bits(getattr(want, name))), (what, name)
    assert np.array_equal(bits(host(weight)), bits(want.weight)), what
    assert np.array_equal(bits(host(cweight)), bits(want.color_weight)), what
    assert int(rows_.count) == want.count and int(rows_.color_count) == want.color_count, what


def same_scaled(got, want, what=""):
    """(pose, trace, deltas, cdeltas) of the device against the restatement, bit for bit"""
    same_solve(got[:2], want[:2], what)
    assert np.array_equal(bits(host(got[2])), bits(want[2])), (what, "deltas", host(got[2]), want[2])
    assert np.array_equal(bits(host(got[3])), bits(want[3])), (what, "cdeltas", host(got[3]), want[3])


# ------------------------------------------------------------------------------------------ 1. the selection alone
# (h, w, coloured count or None = every interior pixel): 1, 2 and the counts around the 256-slot chunk; 513 crosses two
# boundaries; 16 x 17 has 210 interior pixels; 37 * 53 = 1961 slots is no multiple of 4: the tail loop of the select
COUNTS = [(16, 17, 1), (16, 17, 2), (16, 17, None), (37, 53, 255), (37, 53, 256), (37, 53, 257), (37, 53, 513),
          (37, 53, None)]


def used_mask(h, w, n, rng):
    """n interior pixels (None: all of them), which are the ones that can be coloured, and every second border pixel,
    which is used and has no colour row"""
    inner = csr.interior(h, w).reshape(-1)
    ids = np.nonzero(inner)[0]
    used = np.zeros(h * w, bool)
    used[ids if n is None else rng.permutation(ids)[:n]] = True
    used[np.nonzero(~inner)[0][::2]] = True
    return used, int(ids.size if n is None else n)


@pytest.mark.parametrize("name", MULTISETS)
def test_selection_alone_through_the_rows_entry(ops, name):
    rng = np.random.default_rng(13)
    for h, w, n in COUNTS:
        used, n = used_mask(h, w, n, rng)
        e = _multiset(name, h * w, rng)
        fx = csr.residual_fixture(h, w, e, used)
        a = pcr.args_of(fx)
        what = (name, h, w, n)
        want = csr.rows(*a, fx["T"], 1.0, color_huber_k=K)
        col = want.colored
        # the colour residuals are exactly the chosen ones, on exactly the intended slots; color_weight 1: bc == r
        assert col.sum() == n and np.array_equal(col, used & csr.interior(h, w).reshape(-1)), what
        assert np.array_equal(want.code == 0, used) and (want.b == 0).all(), what
        assert np.array_equal(bits(want.r[col]), bits(e[col])) and np.array_equal(bits(want.bc), bits(want.r)), what
        med = np.sort(np.abs(e[col]))[(n - 1) // 2]
        assert bits(want.cdelta) == bits(sr.constant(K) * med), what
        t, _ = geo(fx)
        kw = dict(color_weight=1.0, return_weights=True)
        same_rows(ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_huber_k=K, **kw), want, what)
        if want.cdelta == 0:       # a median of 0: floor 0, every colour weight 1, the unweighted call's sums
            plain = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_weight=1.0)
            assert np.array_equal(want.color_weight, col.astype(F))
            assert np.array_equal(bits(want.sums), bits(host(plain.sums))), what
        if name == "mostly zeros" and n > 2:
            assert want.cdelta == 0, what
        # a floor above the product takes its place
        floor = 2.0 * float(want.cdelta) + 0.5
        high = csr.rows(*a, fx["T"], 1.0, color_huber_k=K, color_huber_delta=floor)
        assert bits(high.cdelta) == bits(F(floor))
        same_rows(ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_huber_k=K, color_huber_delta=floor,
                                                **kw), high, what + ("floor",))


def test_no_coloured_slot_reports_the_floor(ops):
    """ok = 0 everywhere, geometric inliers present: cdelta is the floor and the sums are those without the constant"""
    h, w = 16, 17
    e = np.full(h * w, 2.0 ** -6, F)
    fx = csr.residual_fixture(h, w, e, np.ones(h * w, bool), ok=np.zeros((h, w), bool))
    t, _ = geo(fx)
    kw = dict(color_weight=1.0, return_weights=True, color_huber_delta=0.03)
    want = csr.rows(*pcr.args_of(fx), fx["T"], 1.0, color_huber_k=K, color_huber_delta=0.03)
    assert want.count == h * w and want.color_count == 0 and bits(want.cdelta) == bits(F(0.03))
    got = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_huber_k=K, **kw)
    same_rows(got, want)
    off = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), **kw)
    assert np.array_equal(bits(host(got[0].sums)), bits(host(off[0].sums)))
    # ... and with the geometric rule next to it, whose own n > 0
    both = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_huber_k=K, huber_k=K, huber_delta=1e-3, **kw)
    same_rows(both, csr.rows(*pcr.args_of(fx), fx["T"], 1.0, K, 1e-3, K, 0.03))


# ------------------------------------------------------------------------------------------ 3. rows and solve
# (huber_k, huber_delta, color_huber_k, color_huber_delta): the colour rule alone, with a constant geometric threshold,
# with the geometric rule, and both rules with floors
COMBOS = {"colour rule alone": (0.0, 0.0, K, 0.0), "constant huber_delta": (0.0, 0.005, K, 0.0),
          "both rules": (K, 0.0, K, 0.0), "both rules with floors": (K, 0.004, K, 0.05)}


@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("h,w,stride", [(37, 53, 3), (60, 80, 1), (60, 80, 4)])
def test_rows_and_solve_bit_for_bit(ops, h, w, stride, combo):
    fx = color_edge_fixture(h, w, stride)
    hk, hd, ck, cd = COMBOS[combo]
    n = 6 if h == 37 else 8
    a = pcr.args_of(fx)
    what = "%dx%d stride %d %s" % (h, w, stride, combo)
    t, n_dev = geo(fx)
    huber = dict(huber_k=hk, huber_delta=hd, color_huber_k=ck, color_huber_delta=cd)
    # one linearisation, 4 cm off
    r = csr.rows(*a, fx["T"], WEIGHT, hk, hd, ck, cd, stride=stride)
    assert (r.color_weight[r.colored] < 1).sum() >= 5 and (r.color_weight[r.colored] == 1).sum() >= 5, what
    got = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_weight=WEIGHT, n_dev=n_dev, stride=stride,
                                        return_weights=True, **huber)
    same_rows(got, r, what)
    only = ops.projective_icp_color_rows(*t, dev(fx["T"]), *colour(fx), color_weight=WEIGHT, n_dev=n_dev, stride=stride,
                                         **huber)
    assert isinstance(only, ops.ProjectiveColorRows) and np.array_equal(bits(host(only.sums)), bits(r.sums)), what
    # the solve
    want = csr.color_solve(*a, fx["T0"], WEIGHT, hk, hd, ck, cd, stride=stride, numiters=n)
    const = rr.color_solve(*a, fx["T0"], WEIGHT, hd, cd, stride=stride, numiters=n)
    assert not np.array_equal(want[0], const[0]) and np.unique(want[3]).size > 1, what
    kw = dict(color_weight=WEIGHT, n_dev=n_dev, stride=stride, numiters=n, return_trace=True, **huber)
    got = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), return_scale=True, return_color_scale=True, **kw)
    same_scaled(got, want, what)
    assert got[2].shape == (n,) and got[3].shape == (n,)
    same_solve(ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), **kw), want[:2], what + " without the thresholds")
    T, trace, cdeltas = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), return_color_scale=True, **kw)
    same_solve((T, trace), want[:2], what)
    assert np.array_equal(bits(host(cdeltas)), bits(want[3])), what


# ------------------------------------------------------------------------------------------ 4. independence
def joint_entry(ops, fx, stride, numiters, hk, hd, ck, cd, want_deltas=True):
    """gs_projective_icp_color_joint_scaled_batch_f32 itself, whatever the constants (the Python layer goes there only
    with color_huber_k > 0): (pose, trace, deltas or None)"""
    from gradslam_amd import _C
    t, n_dev = geo(fx)
    b = lambda x: x.unsqueeze(0)      # noqa: E731
    who = "projective_icp_color"
    seqs, held, device, Bn, H, W = ops._picp_seqs(who, b(t[0]), b(t[1]), b(t[2]), b(t[3]), b(t[4]), b(t[5]),
                                                  [(t[6], t[7], None, n_dev)], b(dev(fx["T0"])))
    ops._picp_scratch(seqs, device, "joint_scaled", H, W, stride)
    cseqs = ops._picp_color_seqs(who, seqs, held, Bn, H, W, b(dev(fx["color"])), b(dev(fx["model"])))
    opt = ops._picp_options(who, geometry=(stride, numiters, 1e-8, 0.1, 30.0))
    T, trace, prm = ops._picp_outputs(who, [c.base for c in cseqs], device, None, True, ops.PICP_COLOR_TRACE, opt)
    scale, dptrs = ops._picp_scale_table(Bn, numiters, device) if want_deltas else (None, None)
    _C.check(_C.lib().gs_projective_icp_color_joint_scaled_batch_f32(cseqs, dptrs, None, Bn, H, W, prm, WEIGHT, hk, hd, ck,
                                                                     cd, _C.stream(device)), "joint scaled")
    torch.cuda.synchronize()
    return T[0], trace[0], None if scale is None else scale[0]


@pytest.mark.parametrize("h,w,stride", [(37, 53, 3), (60, 80, 4)])
def test_a_constant_of_zero_leaves_what_ran_before(ops, h, w, stride):
    fx = color_edge_fixture(h, w, stride)
    n = 5
    t, n_dev = geo(fx)
    kw = dict(color_weight=WEIGHT, n_dev=n_dev, stride=stride, numiters=n, return_trace=True)
    # the geometric rule alone: the new entry and gs_projective_icp_color_scaled_batch_f32
    old = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), huber_k=K, huber_delta=1e-3, color_huber_delta=0.02,
                                   return_scale=True, **kw)
    new = joint_entry(ops, fx, stride, n, K, 1e-3, 0.0, 0.02)
    for g, w_ in zip(new, old):
        assert np.array_equal(bits(host(g)), bits(host(w_)))
    same_solve(old[:2], sr.color_solve(*pcr.args_of(fx), fx["T0"], WEIGHT, K, 1e-3, 0.02, stride=stride, numiters=n)[:2])
    # both constants 0: the constant-threshold solve and the plain one
    const = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), huber_delta=0.005, color_huber_delta=0.02, **kw)
    new = joint_entry(ops, fx, stride, n, 0.0, 0.005, 0.0, 0.02, want_deltas=False)
    assert np.array_equal(bits(host(new[0])), bits(host(const[0]))) and np.array_equal(bits(host(new[1])),
                                                                                       bits(host(const[1])))
    plain = pcr.solve(*pcr.args_of(fx), fx["T0"], WEIGHT, stride=stride, numiters=n)
    same_solve(ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), **kw), plain, "no keyword")
    got = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), huber_k=0.0, color_huber_k=0.0, return_scale=True,
                                   return_color_scale=True, color_huber_delta=0.0, **kw)
    same_solve(got[:2], plain, "both constants 0")
    assert (host(got[2]) == 0).all() and (host(got[3]) == 0).all()
    off = ops.projective_icp_color(*t, dev(fx["T0"]), *colour(fx), color_huber_delta=0.02, return_color_scale=True, **kw)
    assert (host(off[2]) == F(0.02)).all() and off[2].shape == (n,)      # color_huber_k 0: the constant in every entry
    new = joint_entry(ops, fx, stride, n, 0.0, 0.0, 0.0, 0.0, want_deltas=False)
    same_solve(new[:2], plain, "the new entry with everything 0")


# ------------------------------------------------------------------------------------------ 5. batch
def nine_sequences():
    """three scenes, each with three masks on the model view's ok channel: different coloured counts, sequence 4 with
    none at all"""
    base = three_sequences()
    seqs = []
    for i in range(9):
        q = dict(base[i % 3])
        model = np.array(q["model"])
        if i == 4:
            model[..., 1:] = 0.0
        elif i >= 3:
            model[:, (i * 7) % 40:(i * 7) % 40 + 25, 1:] = 0.0
        q["model"] = model
        seqs.append(q)
    return seqs


def test_batch_of_nine_crosses_the_launch_boundary(ops):
    """B = 9: 8 sequences per launch (a select grid of 16 blocks with both rules), the ninth goes through launches of
    its own; every sequence has its own thresholds and equals its lone solve"""
    seqs = nine_sequences()
    kw = dict(stride=4, numiters=4, huber_k=K, color_huber_k=K, return_scale=True, return_color_scale=True)
    T, trace, scale, cscale = batch_call(ops, seqs, **kw)
    assert scale.shape == (9, 4) and cscale.shape == (9, 4)
    counts = host(trace)[:, 0, 8]
    assert counts[4] == 0 and np.unique(counts).size >= 6 and (host(cscale)[4] == 0).all()
    assert (host(cscale)[np.arange(9) != 4] > 0).all()
    for i, q in enumerate(seqs):
        lone = solve_hip(ops, q, **kw)
        for g, l_ in zip((T[i], trace[i], scale[i], cscale[i]), lone):
            assert np.array_equal(bits(host(g)), bits(host(l_))), i
    for i in (1, 4, 8):
        want = csr.color_solve(*pcr.args_of(seqs[i]), seqs[i]["T0"], WEIGHT, K, 0.0, K, 0.0, stride=4, numiters=4)
        same_scaled((T[i], trace[i], scale[i], cscale[i]), want, "sequence %d" % i)
    # the colour rule alone: a select grid of B blocks on the second set of tables
    T1, trace1, cscale1 = batch_call(ops, seqs, stride=4, numiters=4, color_huber_k=K, return_color_scale=True)
    want = csr.color_solve(*pcr.args_of(seqs[8]), seqs[8]["T0"], WEIGHT, color_huber_k=K, stride=4, numiters=4)
    same_solve((T1[8], trace1[8]), want[:2], "colour rule alone, sequence 8")
    assert np.array_equal(bits(host(cscale1[8])), bits(want[3]))


# ------------------------------------------------------------------------------------------ 6. the same scratch again
def test_two_solves_in_a_row_on_the_same_scratch_give_the_same_bits(ops):
    """each select block leaves its own counters cleared, both sets: a second solve, and a solve with the other set of
    rules in between, change nothing"""
    fx = color_edge_fixture(60, 80, 4)
    kw = dict(stride=4, numiters=5, return_scale=True, return_color_scale=True)
    both = dict(huber_k=K, color_huber_k=K)
    first = solve_hip(ops, fx, **both, **kw)
    second = solve_hip(ops, fx, **both, **kw)
    solve_hip(ops, fx, color_huber_k=K, **kw)
    solve_hip(ops, fx, huber_k=K, **kw)
    third = solve_hip(ops, fx, **both, **kw)
    for again in (second, third):
        for g, w_ in zip(again, first):
            assert np.array_equal(bits(host(g)), bits(host(w_)))
    seqs = nine_sequences()
    a = batch_call(ops, seqs, stride=4, numiters=3, **both, **{k: kw[k] for k in ("return_scale", "return_color_scale")})
    b = batch_call(ops, seqs, stride=4, numiters=3, **both, **{k: kw[k] for k in ("return_scale", "return_color_scale")})
    for g, w_ in zip(a, b):
        assert np.array_equal(bits(host(g)), bits(host(w_)))


# ------------------------------------------------------------------------------------------ 7. provider and drivers
@pytest.mark.parametrize("which", ["PointFusion", "ICPSLAM"])
def test_drivers_with_the_colour_rule_equal_the_hand_written_loop(gs, ops, which):
    kw = dict(color_huber_k=K)
    want = hand_written_loop(gs, ops, which, textured_frames(gs), weight=1.0, **kw)
    plain = hand_written_loop(gs, ops, which, textured_frames(gs), weight=1.0)
    assert not np.array_equal(host(want[1]), host(plain[1]))                  # the rule reaches the solve
    same_run(make_slam(gs, which, color_weight=1.0, **kw)(textured_frames(gs)), want)


def test_driver_with_both_rules_equals_the_hand_written_loop(gs, ops):
    kw = dict(huber_k=K, color_huber_k=K, color_huber_delta=0.01)
    want = hand_written_loop(gs, ops, "PointFusion", textured_frames(gs), weight=1.0, **kw)
    one = hand_written_loop(gs, ops, "PointFusion", textured_frames(gs), weight=1.0, huber_k=K, color_huber_delta=0.01)
    assert not np.array_equal(host(want[1]), host(one[1]))
    same_run(make_slam(gs, "PointFusion", color_weight=1.0, **kw)(textured_frames(gs)), want)
