"""GPU tests of the ordered mode of the projective ICP's backward pass (gs_picp_bwd.hip, RECORD instances + settle step
-> gs_projective_icp_ordered_backward_batch_f32 -> ops.projective_icp_backward_batch(deterministic=True) ->
ProjectiveICPFunction -> ProjectiveICPOdometryProvider(deterministic_backward=True) -> PointFusion(
odom_deterministic_backward=True)).

The arbiter of the map gradients' BITS is the order contract restated in tests/picp_ordered_ref.py, applied to the keys
and contributions the kernel recorded; that the record is the right one is checked against the NumPy forward's
association (the keys) and against the float64 adjoint (the sums, within kernel_bound(gap): the bar of the atomic mode,
tests/test_hip_picp_backward.py).  Everything the atomic mode makes reproducible keeps its bits."""
import numpy as np
import pytest
import torch

from tests import backward_cases as bc
from tests import picp_backward_cases as pc
from tests import picp_ordered_ref as orf
from tests import picp_robust_backward_cases as rc
from tests import picp_scale_backward_cases as sc
from tests.test_hip_picp import FUSION, bits, dev, frames_of, host

pytestmark = pytest.mark.gpu

SMALL = ("edge_s3", "conv_s4", "radius1", "stale_dc", "conv_s4_n1")     # (not conv_t2: 66 049 slots)
KNOB = "GRADSLAM_HIP_DETERMINISTIC_BACKWARD"


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


# ------------------------------------------------------------------------------------------ the ops-level harness
class Tape:
    """the device tensors of B sequences and the tape of their forward"""


def tape_of(ops, fxs, counts, stride, numiters, kw, huber_delta=0.0, huber_k=0.0):
    st = lambda k: torch.stack([dev(q[k]) for q in fxs])   # noqa: E731
    t = Tape()
    t.args = [st(k) for k in ("vertex", "normal", "depth", "K", "index", "model_pose")]
    t.maps = [(dev(q["points"]), dev(q["normals"]), None,
               None if n is None else torch.tensor([n], dtype=torch.int64, device="cuda")) for q, n in zip(fxs, counts)]
    t.kw = dict(stride=stride, numiters=numiters, huber_delta=huber_delta, huber_k=huber_k, **kw)
    t.tapes = torch.empty((len(fxs), ops.projective_icp_tape_bytes(numiters)), dtype=torch.uint8, device="cuda")
    opt = ops._picp_options("projective_icp", geometry=(stride, numiters, kw["damp"], kw["dist_thresh"],
                                                        kw["angle_thresh"]), huber_delta=huber_delta, huber_k=huber_k)
    t.pose = ops._picp_solve(opt, *t.args, t.maps, st("T0"), tapes=t.tapes)
    return t


def case_tape(ops, c, **extra):
    return tape_of(ops, [c.fx], [c.device_count], c.stride, c.numiters, c.kw, **extra)


def backward(ops, t, T_bars, deterministic=True, record=False, **want):
    """[per sequence (vertex_bar, points_bar, normals_bar, init_pose_bar)] as host arrays (None where not wanted), and with
    record the per-sequence (keys, contrib)"""
    res = ops.projective_icp_backward_batch(*t.args, t.maps, t.tapes, torch.stack([dev(x) for x in T_bars]),
                                            deterministic=deterministic, return_contributions=record, **t.kw, **want)
    torch.cuda.synchronize()
    vb, rows, ib = res[:3]
    h = lambda x: None if x is None else host(x)   # noqa: E731
    out = [(None if vb is None else host(vb[b]), h(rows[b][0]), h(rows[b][1]), None if ib is None else host(ib[b]))
           for b in range(len(rows))]
    if record:
        return out, [(host(k), host(c)) for k, c in res[3]]
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def restated(keys, contrib, got):
    """the map gradients of a sequence against the order contract applied to its record, bit for bit"""
    Pb, Nb = orf.ordered_sum(keys, contrib, got[1].shape[0])
    assert same_bits(got[1], Pb), "points_bar left the order contract"
    assert same_bits(got[2], Nb), "normals_bar left the order contract"


def witnesses(c, keys):
    """what the record of a case must show for the comparison to mean something (asserted from the returned keys)"""
    used = keys != orf.NO_KEY
    most = max(int(np.bincount(k[u]).max()) for k, u in zip(keys, used) if u.any())
    assert most >= (4 if c.name == "radius1" else 2), "%s: no row with several contributions in one iteration" % c.name
    if c.numiters > 1:
        per_it = [set(k[u].tolist()) for k, u in zip(keys, used)]
        assert any(per_it[i] & per_it[j] for i in range(len(per_it)) for j in range(i)), "no row in two iterations"
    count = c.device_count if c.device_count is not None else c.fx["points"].shape[0]
    assert keys[used].max() < count and keys[used].min() >= 0
    want = np.where(c.assoc.used, c.assoc.rows, orf.NO_KEY)
    assert keys.shape == want.shape and np.array_equal(keys, want), "the recorded keys are not the forward's association"


# ------------------------------------------------------------------------------------------ 1, 2, 3: bits, bar, the rest
@pytest.mark.parametrize("name", SMALL)
def test_bits_against_the_restatement_and_the_float64_adjoint(ops, name):
    """edge_s3: 234 slots = one partial chunk, every reject code; conv_s4: 300 slots = a full chunk + a tail; radius1: a
    row behind >= 4 slots; stale_dc: stale index entries behind a device-side count; conv_s4_n1: numiters = 1."""
    c = pc.build(name)
    pc.claims(c)
    t = case_tape(ops, c)
    assert same_bits(host(t.pose[0]), c.assoc.pose), "the taped forward left the restated solve"
    (got,), ((keys, contrib),) = backward(ops, t, [c.T_bar], record=True)
    assert keys.dtype == np.int32 and contrib.dtype == np.float64 and contrib.shape == keys.shape + (6,)
    assert keys.shape == (c.numiters, c.v.shape[0])
    restated(keys, contrib, got)
    witnesses(c, keys)
    # 2. the same adjoint, the atomic mode's bar
    want = pc.reference(c)
    for out, g, w, gap in zip(pc.OUTPUTS, got, want, pc.GAP[name]):
        err, bound = bc.rel_err(g, w), bc.kernel_bound(gap)
        print("%s %s: rel_err %.3g, bound %.3g (gap %.2g)" % (name, out, err, bound, gap))
    for out, g, w, gap in zip(pc.OUTPUTS, got, want, pc.GAP[name]):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, out)
        assert bc.rel_err(g, w) <= bc.kernel_bound(gap), (name, out, bc.rel_err(g, w), bc.kernel_bound(gap))
    if c.device_count is not None:   # rows at and beyond the device count are never touched: +0.0
        assert (bits(got[1][c.device_count:]) == 0).all() and (bits(got[2][c.device_count:]) == 0).all()
    # 3. the rest does not move
    (atomic,) = backward(ops, t, [c.T_bar], deterministic=False)
    assert same_bits(got[0], atomic[0]) and same_bits(got[3], atomic[3])
    assert np.abs(got[1]).max() > 0 and np.abs(got[2]).max() > 0


# ------------------------------------------------------------------------------------------ 4. reproducible
def test_two_calls_and_a_call_after_another_case_give_the_same_bits(ops):
    c, other = pc.build("conv_s4"), pc.build("radius1")
    t, t2 = case_tape(ops, c), case_tape(ops, other)
    (a,) = backward(ops, t, [c.T_bar])
    (b,) = backward(ops, t, [c.T_bar])
    backward(ops, t2, [other.T_bar])          # (more slots, more rows: whatever it leaves in the scratch must not show)
    (d,) = backward(ops, t, [c.T_bar])
    for i in range(4):
        assert same_bits(a[i], b[i]) and same_bits(a[i], d[i]), pc.OUTPUTS[i]


# ------------------------------------------------------------------------------------------ 5. no inliers
@pytest.mark.parametrize("name", pc.NO_INLIER)
def test_no_inlier_records_nothing(ops, name):
    c = pc.build(name)
    T_bar = c.T_bar.copy()
    T_bar[1, 2], T_bar[2, 3] = -0.0, -0.0
    t = case_tape(ops, c)
    (got,), ((keys, contrib),) = backward(ops, t, [T_bar], record=True)
    assert (keys == orf.NO_KEY).all()
    assert (bits(got[0]) == 0).all() and (bits(got[1]) == 0).all() and (bits(got[2]) == 0).all()
    assert same_bits(got[3][:3], T_bar[:3]) and (bits(got[3][3]) == 0).all()
    restated(keys, contrib, got)


def test_a_sequence_without_inliers_next_to_one_with(ops):
    """conv_s4 twice, the second with an index image of -1: its keys all read "none" in every iteration (not what the
    first iteration's launch or the other sequence left), and the first sequence has the bits of its single call"""
    c = pc.build("conv_s4")
    blind = dict(c.fx, index=np.full_like(c.fx["index"], -1))
    T_bars = [c.T_bar, bc.weights((4, 4), 32)]
    t = tape_of(ops, [c.fx, blind], [c.device_count] * 2, c.stride, c.numiters, c.kw)
    got, rec = backward(ops, t, T_bars, record=True)
    (single,), ((skeys, scontrib),) = backward(ops, case_tape(ops, c), T_bars[:1], record=True)
    for i in range(4):
        assert same_bits(got[0][i], single[i]), pc.OUTPUTS[i]
    assert np.array_equal(rec[0][0], skeys)
    restated(rec[0][0], rec[0][1], got[0])
    assert (rec[1][0] == orf.NO_KEY).all()
    assert all((bits(g) == 0).all() for g in got[1][:3])
    assert same_bits(got[1][3][:3], T_bars[1][:3])
    # ... and the other way round: the blind sequence first
    t = tape_of(ops, [blind, c.fx], [c.device_count] * 2, c.stride, c.numiters, c.kw)
    got = backward(ops, t, T_bars[::-1])
    for i in range(4):
        assert same_bits(got[1][i], single[i]), pc.OUTPUTS[i]
    assert all((bits(g) == 0).all() for g in got[0][:3])


# ------------------------------------------------------------------------------------------ 6. batches
def three_cases():
    """three 60 x 80 fixtures of the cases with maps of three sizes: conv_s4's, stale_dc's (another scene; buffers cut to
    100 rows beyond its device count, which no slot may read) and radius1's in buffers seven rows longer than its count"""
    a, b, r = pc.build("conv_s4"), pc.build("stale_dc"), pc.build("radius1")
    pad = lambda x: np.concatenate([x, np.full((7, 3), np.nan, np.float32)])   # noqa: E731
    fr = dict(r.fx, points=pad(r.fx["points"]), normals=pad(r.fx["normals"]))
    keep = b.device_count + 100
    fb = dict(b.fx, points=b.fx["points"][:keep], normals=b.fx["normals"][:keep])
    fxs, counts = [a.fx, fb, fr], [a.device_count, b.device_count, r.fx["points"].shape[0]]
    assert len({q["points"].shape[0] for q in fxs}) == 3
    return fxs, counts


def test_batch_of_three_equals_three_single_calls(ops):
    fxs, counts = three_cases()
    kw = dict(pc.KW, dist_thresh=0.5)
    T_bars = [bc.weights((4, 4), 40 + b) for b in range(3)]
    got, rec = backward(ops, tape_of(ops, fxs, counts, 4, 5, kw), T_bars, record=True)
    shared = 0
    for b in range(3):
        (single,) = backward(ops, tape_of(ops, fxs[b:b + 1], counts[b:b + 1], 4, 5, kw), T_bars[b:b + 1])
        for i in range(4):
            assert same_bits(got[b][i], single[i]), (b, pc.OUTPUTS[i])
        restated(rec[b][0], rec[b][1], got[b])
        assert np.abs(got[b][1]).max() > 0 and np.abs(got[b][2]).max() > 0
        shared = max(shared, max(int(np.bincount(k[k != orf.NO_KEY]).max()) for k in rec[b][0]))
    assert shared >= 2, "no row with several contributions: the batch could not tell the orders apart"


def test_batch_of_nine_crosses_the_launch_group(ops):
    """8 sequences per launch group and per sort: the ninth goes through launches and a sort of its own"""
    c = pc.build("conv_s4")
    T_bars = [bc.weights((4, 4), 50 + i) for i in range(9)]
    got = backward(ops, tape_of(ops, [c.fx] * 9, [c.device_count] * 9, c.stride, 4, c.kw), T_bars)
    t1 = tape_of(ops, [c.fx], [c.device_count], c.stride, 4, c.kw)
    for i in range(9):
        (single,) = backward(ops, t1, T_bars[i:i + 1])
        for j in range(4):
            assert same_bits(got[i][j], single[j]), (i, pc.OUTPUTS[j])
    assert not same_bits(got[0][1], got[8][1])


# ------------------------------------------------------------------------------------------ 7. outputs not asked for
def test_outputs_not_asked_for(ops):
    c = pc.build("conv_s4")
    t = case_tape(ops, c)
    (full,) = backward(ops, t, [c.T_bar])
    (atomic,) = backward(ops, t, [c.T_bar], deterministic=False, want_maps=[(False, False)])
    (none,) = backward(ops, t, [c.T_bar], want_maps=[(False, False)])
    assert none[1] is None and none[2] is None
    assert same_bits(none[0], atomic[0]) and same_bits(none[3], atomic[3]) and same_bits(none[0], full[0])
    (maps_only,) = backward(ops, t, [c.T_bar], want_vertex=False, want_init=False)
    assert maps_only[0] is None and maps_only[3] is None
    assert same_bits(maps_only[1], full[1]) and same_bits(maps_only[2], full[2])
    # points for one sequence, normals for the other
    t2 = tape_of(ops, [c.fx] * 2, [c.device_count] * 2, c.stride, c.numiters, c.kw)
    both = backward(ops, t2, [c.T_bar] * 2)
    part, rec = backward(ops, t2, [c.T_bar] * 2, want_maps=[(True, False), (False, True)], record=True)
    assert part[0][2] is None and part[1][1] is None
    assert same_bits(part[0][1], both[0][1]) and same_bits(part[0][1], full[1])
    assert same_bits(part[1][2], both[1][2]) and same_bits(part[1][2], full[2])
    u0, u1 = rec[0][0] != orf.NO_KEY, rec[1][0] != orf.NO_KEY       # (a contribution is defined where the key is a row)
    assert u0.any() and u1.any()
    assert (rec[0][1][u0][:, 3:] == 0).all() and (rec[1][1][u1][:, :3] == 0).all()   # the half not asked for: zeros
    assert (rec[0][1][u0][:, :3] != 0).any() and (rec[1][1][u1][:, 3:] != 0).any()
    # one sequence with map outputs, one without: the one without records nothing
    part, rec = backward(ops, t2, [c.T_bar] * 2, want_maps=[(False, False), (True, True)], record=True)
    assert (rec[0][0] == orf.NO_KEY).all() and same_bits(part[1][1], full[1]) and same_bits(part[1][2], full[2])
    assert same_bits(part[0][0], full[0]) and same_bits(part[0][3], full[3])


# ------------------------------------------------------------------------------------------ 8. robust and scaled tapes
@pytest.mark.parametrize("which", ["robust", "scaled"])
def test_robust_and_scaled_tapes(ops, which):
    # edge_s1's fixture: 1 961 slots = 7 chunks and a tail, a device count, rows that recur from one iteration to the next
    # (conv_s4 moves every slot to another surfel between its two robust iterations: no such row)
    if which == "robust":
        c = rc.build("edge_s1", 0.005)
        assert c.delta == 0.005
        extra, clipped = dict(huber_delta=c.delta), c.assoc.clipped
    else:
        c = sc.build("edge_s1")
        assert c.huber_k == 1.345
        extra, clipped = dict(huber_k=c.huber_k), c.assoc.clipped
    assert (clipped & c.assoc.used).any() and (~clipped & c.assoc.used).any()      # both branches of the weight
    t = case_tape(ops, c, **extra)
    assert same_bits(host(t.pose[0]), c.assoc.pose), "the taped forward left the restated solve"
    (got,), ((keys, contrib),) = backward(ops, t, [c.T_bar], record=True)
    restated(keys, contrib, got)
    witnesses(c, keys)
    (atomic,) = backward(ops, t, [c.T_bar], deterministic=False)
    assert same_bits(got[0], atomic[0]) and same_bits(got[3], atomic[3])
    if which == "scaled":      # (the committed gap of the case; the robust gaps are those of other thresholds)
        for out, g, w, gap in zip(pc.OUTPUTS, got, sc.reference(c), sc.GAP["edge_s1"]):
            assert bc.rel_err(g, w) <= bc.kernel_bound(gap), (which, out, bc.rel_err(g, w), bc.kernel_bound(gap))


# ------------------------------------------------------------------------------------------ 9. autograd and the drivers
def autograd_run(ops, c, **kw):
    t = {k: dev(c.fx[k]) for k in ("vertex", "normal", "depth", "K", "index", "model_pose", "points", "normals", "T0")}
    for k in ("vertex", "points", "normals", "T0"):
        t[k].requires_grad_(True)
    n_dev = None if c.device_count is None else torch.tensor([c.device_count], dtype=torch.int64, device="cuda")
    T = ops.projective_icp(t["vertex"], t["normal"], t["depth"], t["K"], t["index"], t["model_pose"], t["points"],
                           t["normals"], t["T0"], n_dev=n_dev, stride=c.stride, numiters=c.numiters, differentiable=True,
                           **c.kw, **kw)
    T.backward(dev(c.T_bar))
    torch.cuda.synchronize()
    return [host(t[k].grad) for k in ("vertex", "points", "normals", "T0")]


def test_autograd_and_the_knob(ops, monkeypatch):
    c = pc.build("conv_s4")          # (a 60 x 80 fixture)
    assert c.fx["depth"].shape == (60, 80)
    monkeypatch.delenv(KNOB, raising=False)
    (want,) = backward(ops, case_tape(ops, c), [c.T_bar])
    got = autograd_run(ops, c, deterministic=True)
    for i in range(4):
        assert same_bits(got[i], want[i]), pc.OUTPUTS[i]
    monkeypatch.setenv(KNOB, "1")     # read when the backward runs
    got = autograd_run(ops, c)
    for i in range(4):
        assert same_bits(got[i], want[i]), pc.OUTPUTS[i]
    got = autograd_run(ops, c, deterministic=None)
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    monkeypatch.setenv(KNOB, "0")
    got = autograd_run(ops, c)
    assert same_bits(got[0], want[0]) and same_bits(got[3], want[3])
    ref = pc.reference(c)
    for i in (1, 2):
        assert bc.rel_err(got[i], ref[i]) <= bc.kernel_bound(pc.GAP["conv_s4"][i]), pc.OUTPUTS[i]


def test_point_fusion_twice_from_scratch(gs):
    """three 60 x 80 frames, the map update on the tape, a loss on the last pose: the gradient reaches the depth of the
    earlier frames through the map rows they wrote, i.e. through points_bar / normals_bar of the projective ICP"""
    from gradslam_amd.datasets.synthetic import make_sequence
    sequences = [make_sequence(3, 60, 80, seed=s) for s in (0, 1)]
    Tb = torch.stack([dev(bc.weights((4, 4), 70 + b)) for b in range(2)])

    def run():
        frames = frames_of(gs, sequences)
        frames.depth_image.requires_grad_(True)
        slam = gs.slam.PointFusion(odom="projicp", device="cuda", dsratio=2, numiters=10, odom_differentiable=True,
                                   odom_deterministic_backward=True, **FUSION)
        assert slam.odomprov.deterministic_backward is True
        _, poses = slam(frames)
        assert poses.grad_fn is not None
        (g,) = torch.autograd.grad(poses[:, -1], frames.depth_image, Tb)
        torch.cuda.synchronize()
        return host(poses), host(g)

    p1, g1 = run()
    p2, g2 = run()
    assert same_bits(p1, p2) and same_bits(g1, g2)
    assert np.isfinite(g1).all()
    for s in range(3):
        assert np.abs(g1[:, s]).max() > 0, s
