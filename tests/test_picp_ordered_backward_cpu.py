"""CPU tests of the ordered mode of the projective ICP's backward pass: the restated order contract
(tests/picp_ordered_ref.py) against an independent statement on inputs that tell the orders apart, the new C symbols, the
scratch queries, the argument checks of the new entry (made before any HIP call, so they run without a GPU), the register
report of the new kernels (cross-compiled), the Python layers' switches and the environment knob."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import picp_ordered_ref as orf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gs_projective_icp_ordered_backward_batch_f32"
KNOB = "GRADSLAM_HIP_DETERMINISTIC_BACKWARD"


# ------------------------------------------------------------------------------------------ the restated contract
def order_sensitive_record(seed, numiters=3, nslots=64, n_rows=9):
    """a record whose sums depend on the order: every row gets, per iteration and component, contributions like 1e16,
    1.0, -1e16, 1.0 (times a seeded factor) on slots scattered over the lattice, plus slots without a row"""
    rng = np.random.default_rng(seed)
    keys = np.full((numiters, nslots), orf.NO_KEY, np.int64)
    contrib = rng.standard_normal((numiters, nslots, 6))          # (the entries of unused slots must be ignored)
    for it in range(numiters):
        slots = rng.permutation(nslots)[:4 * (n_rows - 1)].reshape(n_rows - 1, 4)
        for row in range(n_rows - 1):                               # (the last row is never touched)
            ks = np.sort(slots[row])
            scale = rng.uniform(0.5, 2.0, 6)
            for k, v in zip(ks, (1e16, 1.0, -1e16, 1.0)):
                keys[it, k] = row
                contrib[it, k] = v * scale
    return keys, contrib, n_rows


def independent_sum(keys, contrib, n_rows, descending=False):
    """the contract stated another way: per iteration a dict of lists (row -> contributions in slot order), summed with a
    for loop"""
    acc = np.zeros((n_rows, 6), np.float64)
    for it in reversed(range(keys.shape[0])):
        lists = {}
        order = range(keys.shape[1] - 1, -1, -1) if descending else range(keys.shape[1])
        for k in order:
            if keys[it, k] != orf.NO_KEY:
                lists.setdefault(int(keys[it, k]), []).append(contrib[it, k])
        for row, items in lists.items():
            run = np.zeros(6, np.float64)
            for x in items:
                run = run + x
            acc[row] = acc[row] + run
    return acc[:, :3].astype(np.float32), acc[:, 3:].astype(np.float32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ordered_sum_against_an_independent_statement(seed):
    keys, contrib, n_rows = order_sensitive_record(seed)
    got = orf.ordered_sum(keys, contrib, n_rows)
    want = independent_sum(keys, contrib, n_rows)
    other = independent_sum(keys, contrib, n_rows, descending=True)
    for g, w, o in zip(got, want, other):
        assert g.dtype == np.float32 and g.shape == (n_rows, 3)
        assert np.array_equal(g.view(np.int32), w.view(np.int32))
        assert not np.array_equal(g, o), "the inputs cannot tell ascending from descending slot order"
        assert (g[-1].view(np.int32) == 0).all()          # a row that nobody touches: +0.0
    # ascending: (1e16 + 1) - 1e16 + 1 = 1 per iteration (1e16 + 1 rounds to 1e16); descending gives another value
    assert np.abs(got[0][:-1]).max() < 1e3


def test_ordered_sum_of_an_empty_record_is_plus_zero():
    keys = np.full((2, 5), orf.NO_KEY, np.int32)
    contrib = np.full((2, 5, 6), np.nan)
    for g in orf.ordered_sum(keys, contrib, 4):
        assert (g.view(np.int32) == 0).all()


# ------------------------------------------------------------------------------------------ the library
def _lib():
    from gradslam_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from gradslam_amd.csrc import build
        build.build()
    return _C, _C.lib()


def test_new_symbols_are_declared_and_exported():
    _C, lib = _lib()
    names = {ENTRY, "gs_projective_icp_ordered_backward_scratch_bytes",
             "gs_projective_icp_ordered_backward_sort_scratch_bytes"}
    assert names <= set(_C.EXPORTS)
    header = open(os.path.join(REPO, "include", "gradslam_hip.h")).read()
    for n in names:
        assert hasattr(lib, n) and re.search(r"GS_API \w+ %s\(" % n, header), n
    assert "typedef struct gs_picp_ordered_backward_seq" in header and "gs_picp_backward_seq base;" in header
    assert lib.gs_abi_version() == _C.ABI_VERSION == 3          # additions only: the ABI version stays
    assert C.sizeof(_C.PicpOrderedBackwardSeq) == C.sizeof(_C.PicpBackwardSeq) + 16
    assert _C.PicpOrderedBackwardSeq.base.offset == 0


def test_scratch_queries():
    _C, lib = _lib()
    per_seq = lib.gs_projective_icp_ordered_backward_scratch_bytes
    old = lib.gs_projective_icp_backward_scratch_bytes
    sort = lib.gs_projective_icp_ordered_backward_sort_scratch_bytes
    # bad sizes
    assert per_seq(480, 640, 0, 0) == 0 and per_seq(0, 640, 4, 0) == 0 and per_seq(480, 640, 4, -1) == 0
    assert per_seq(46341, 46341, 1, 0) == 0
    assert sort(0, 480, 640, 4) == 0 and sort(1, 480, 640, 0) == 0 and sort(1, 0, 640, 4) == 0
    assert sort(1, 46341, 46341, 1) == 0
    assert sort(8, 20000, 20000, 1) == 0 and sort(1, 20000, 20000, 1) > 0     # 8 x 4e8 pairs >= 2^31: one sort cannot
    for n_map in (0, 1000, 1_000_000):
        assert per_seq(480, 640, 4, n_map) >= old(480, 640, 4, n_map) > 0
    # the record and the keys: at least 48 + 8 bytes per slot between them, the record (48 + 4) with the sequence
    s4, s1 = 120 * 160, 480 * 640
    grow_seq = per_seq(480, 640, 1, 1000) - per_seq(480, 640, 4, 1000)
    grow_old = old(480, 640, 1, 1000) - old(480, 640, 4, 1000)
    grow_sort = sort(1, 480, 640, 1) - sort(1, 480, 640, 4)
    print("per slot: record %.1f, sort buffers %.1f" % ((grow_seq - grow_old) / (s1 - s4), grow_sort / (s1 - s4)))
    assert grow_seq - grow_old >= (48 + 4) * (s1 - s4)
    assert (grow_seq - grow_old) + grow_sort >= (48 + 8) * (s1 - s4)
    assert grow_sort >= 8 * (s1 - s4)
    # the sort buffers hold one launch group: they grow to 8 sequences and no further
    assert sort(8, 480, 640, 4) >= 8 * (8 + 4) * s4 and sort(8, 480, 640, 4) > sort(1, 480, 640, 4)
    assert sort(9, 480, 640, 4) == sort(8, 480, 640, 4) == sort(64, 480, 640, 4)
    # nothing scales with numiters: neither query takes it
    assert len(per_seq.argtypes) == 4 and len(sort.argtypes) == 4


def _filled(_C, lib, H=48, W=64, stride=4, n_bound=100):
    one = C.c_void_p(256)           # (never dereferenced: every check comes before the first HIP call)
    seqs = (_C.PicpOrderedBackwardSeq * 1)()
    u = seqs[0].base
    for f in ("vertex", "normal", "depth", "K16", "index", "model_pose16", "tape", "pose_bar16", "scratch"):
        setattr(u, f, one)
    u.map = _C.MapView(one, one, 0, 0, n_bound, n_bound, 0)
    u.points_bar = one
    u.scratch_bytes = lib.gs_projective_icp_ordered_backward_scratch_bytes(H, W, stride, n_bound)
    return seqs, u, one


def test_entry_checks_its_arguments_before_any_hip_call():
    _C, lib = _lib()
    fn = getattr(lib, ENTRY)
    prm = _C.PicpParams(4, 10, 1e-8, 0.1, 0.8)
    sort_bytes = lib.gs_projective_icp_ordered_backward_sort_scratch_bytes(1, 48, 64, 4)

    def refused(what, seqs, prm=prm, sort=C.c_void_p(512), nbytes=sort_bytes, delta=0.0):
        assert fn(seqs, 1, 48, 64, prm, delta, 0, sort, nbytes, None) == 1, what
        msg = lib.gs_last_error().decode()
        assert msg.startswith(ENTRY + ":") and what in msg, msg

    assert fn(None, 1, 48, 64, prm, 0.0, 0, None, 0, None) == 1 and lib.gs_last_error().decode().startswith(ENTRY)
    empty = (_C.PicpOrderedBackwardSeq * 1)()
    refused("NULL", empty)
    seqs, u, one = _filled(_C, lib)
    refused("NULL", seqs, sort=None)                                   # a map output needs the sort scratch
    refused("sort scratch too small", seqs, nbytes=sort_bytes - 1)
    refused("misaligned sort scratch", seqs, sort=C.c_void_p(516))
    u.scratch_bytes = lib.gs_projective_icp_backward_scratch_bytes(48, 64, 4, 100)   # the atomic mode's: no record
    refused("scratch too small", seqs)
    u.scratch_bytes = lib.gs_projective_icp_ordered_backward_scratch_bytes(48, 64, 4, 0)   # too small for a map output
    refused("scratch too small", seqs)
    seqs, u, one = _filled(_C, lib)
    u.tape = C.c_void_p(260)
    refused("misaligned", seqs)
    seqs, u, one = _filled(_C, lib)
    u.scratch = C.c_void_p(260)
    refused("misaligned", seqs)
    seqs, u, one = _filled(_C, lib)
    refused("stride", seqs, prm=_C.PicpParams(0, 10, 1e-8, 0.1, 0.8))
    refused("huber_delta", seqs, delta=-1.0)
    seqs, u, one = _filled(_C, lib)
    u.map = _C.MapView(one, one, 0, 0, 0x7fffffff, 0x7fffffff, 0)
    u.scratch_bytes = 1 << 62
    refused("0x7fffffff", seqs)
    u.map = _C.MapView(one, one, 0, 0, 0x7ffffffe, 0x7ffffffe, 0)      # the largest map the keys can name is not refused
    u.scratch_bytes = 0                                                 # for its size (but for its scratch)
    refused("scratch too small", seqs)
    # a launch group whose lattices are too many for one sort: 8 sequences of 20 000 x 20 000 slots
    big = (_C.PicpOrderedBackwardSeq * 8)()
    for b in range(8):
        src = _filled(_C, lib)[0][0]
        C.memmove(C.byref(big[b]), C.byref(src), C.sizeof(src))
        big[b].base.scratch_bytes = 1 << 62
    assert fn(big, 8, 20000, 20000, _C.PicpParams(1, 2, 1e-8, 0.1, 0.8), 0.0, 0, C.c_void_p(512), 1 << 62, None) == 1
    msg = lib.gs_last_error().decode()
    assert msg.startswith(ENTRY + ":") and "2^31" in msg, msg


def test_new_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "gs_picp_bwd.hip",
                        "picp_bwd_"], capture_output=True, text=True, cwd=REPO, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split(None, 7)[7].strip(): ln.split(None, 7)[:7] for ln in r.stdout.splitlines()
            if "picp_bwd_" in ln and not ln.startswith("#")}
    new = {"gs_ordered_picp_bwd_point_kernel", "gs_ordered_robust_picp_bwd_point_kernel",
           "gs_ordered_picp_bwd_iota_kernel", "gs_ordered_picp_bwd_settle_kernel"}
    assert new <= set(rows), r.stdout
    # the three kernels of that prefix are still the only ones (tests/test_picp_backward_cpu.py says so too)
    assert {n for n in rows if n.startswith("gs_picp_bwd_")} == \
        {"gs_picp_bwd_scalar_kernel", "gs_picp_bwd_point_kernel", "gs_picp_bwd_cast_kernel"}, r.stdout
    for name in sorted(new):
        vgpr, sgpr, scratch, occ, sspill, vspill, lds = rows[name]
        print(name, "VGPR", vgpr, "scratch", scratch, "occupancy", occ, "LDS", lds)
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, vspill, sspill)
    # the RECORD parameter left the atomic instances with the registers the existing test pins
    assert int(rows["gs_picp_bwd_point_kernel"][0]) <= 128 and int(rows["gs_picp_bwd_point_kernel"][3]) >= 4


# ------------------------------------------------------------------------------------------ the Python layers
def _cpu_args(H=4, W=5):
    return [torch.zeros(H, W, 3), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(4),
            torch.zeros(H, W, dtype=torch.int64), torch.eye(4), torch.zeros(3, 3), torch.zeros(3, 3), torch.eye(4)]


def _backward_args(H=4, W=5):
    a = _cpu_args(H, W)
    return [a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None], [(a[6], a[7], None, None)],
            torch.zeros(1, 328, dtype=torch.uint8), a[8][None]]


def test_ops_accept_and_type_check_the_switch(monkeypatch):
    from gradslam_amd import _C, ops
    monkeypatch.delenv(KNOB, raising=False)
    a = _cpu_args()
    for bad in (1, "yes", 0.0):
        with pytest.raises(TypeError, match="deterministic"):
            ops.projective_icp(*a, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic"):
            ops.projective_icp(*a, differentiable=True, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic"):
            ops.projective_icp_batch(a[0][None], a[1][None], a[2][None], a[3][None], a[4][None], a[5][None],
                                     [(a[6], a[7], None, None)], a[8][None], deterministic=bad)
        with pytest.raises(TypeError, match="deterministic"):
            ops.projective_icp_backward_batch(*_backward_args(), numiters=1, deterministic=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="return_contributions"):
            ops.projective_icp_backward_batch(*_backward_args(), numiters=1, deterministic=True, return_contributions=bad)
    for ok in (None, True, False):      # accepted: what stops the call is the missing device, not the switch
        with pytest.raises(_C.HipExtensionError):
            ops.projective_icp(*a, differentiable=True, deterministic=ok)
        with pytest.raises(_C.HipExtensionError):
            ops.projective_icp_backward_batch(*_backward_args(), numiters=1, deterministic=ok)
    for off in (None, False):
        with pytest.raises(ValueError, match="return_contributions"):
            ops.projective_icp_backward_batch(*_backward_args(), numiters=1, deterministic=off, return_contributions=True)
    monkeypatch.setenv(KNOB, "1")       # the knob switches the ordered mode on: the same call now gets to the device check
    with pytest.raises(_C.HipExtensionError):
        ops.projective_icp_backward_batch(*_backward_args(), numiters=1, return_contributions=True)
    with pytest.raises(ValueError, match="return_contributions"):      # ... and an explicit False wins over it
        ops.projective_icp_backward_batch(*_backward_args(), numiters=1, deterministic=False, return_contributions=True)


def test_provider_and_drivers_accept_and_type_check_the_switch():
    import gradslam_amd as gs
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    assert ProjectiveICPOdometryProvider().deterministic_backward is None
    for ok in (None, True, False):
        p = ProjectiveICPOdometryProvider(differentiable=True, deterministic_backward=ok)
        assert p.deterministic_backward is ok
        assert "deterministic" not in "".join(p._kwargs())      # carried next to _kwargs(), like color_weight
    for bad in (1, "yes"):
        with pytest.raises(TypeError, match="deterministic_backward"):
            ProjectiveICPOdometryProvider(deterministic_backward=bad)
    for cls in (gs.slam.ICPSLAM, gs.slam.PointFusion):
        s = cls(odom="projicp")
        assert s.odom_deterministic_backward is None and s.odomprov.deterministic_backward is None
        for ok in (True, False):
            s = cls(odom="projicp", odom_differentiable=True, odom_deterministic_backward=ok)
            assert s.odom_deterministic_backward is ok and s.odomprov.deterministic_backward is ok
        for bad in (1, "yes"):
            with pytest.raises(TypeError, match="odom_deterministic_backward"):
                cls(odom="projicp", odom_deterministic_backward=bad)
        for ok in (True, False):
            with pytest.raises(ValueError, match="projicp"):
                cls(odom="gradicp", odom_deterministic_backward=ok)
        assert cls(odom="gradicp").odom_deterministic_backward is None


def test_the_knob_is_read_per_call_with_the_rule_of_atoi(monkeypatch):
    from gradslam_amd import ops
    got = []
    for val in ("1", "0", "2", "x", None):
        if val is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, val)
        got.append(ops.deterministic_backward_env())
    assert got == [True, False, True, False, False]
    # C atoi: leading white space and a sign are skipped, the digits up to the first other character count
    libc = C.CDLL(None)
    for val in ("", " 1", "+1", "-1", "01", "1x", "x1", "0x10", "1.5", "0.5", " \t3", "--1", "+ 1", "00"):
        monkeypatch.setenv(KNOB, val)
        assert ops.deterministic_backward_env() == (libc.atoi(val.encode()) != 0), repr(val)
    # ... and per call: the ordered mode is what makes return_contributions legal
    monkeypatch.setenv(KNOB, "0")
    with pytest.raises(ValueError, match="return_contributions"):
        ops.projective_icp_backward_batch(*_backward_args(), numiters=1, return_contributions=True)
    monkeypatch.setenv(KNOB, "1")
    from gradslam_amd import _C
    with pytest.raises(_C.HipExtensionError):
        ops.projective_icp_backward_batch(*_backward_args(), numiters=1, return_contributions=True)
