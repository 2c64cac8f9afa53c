"""CPU tests of the guarded, exact workspace (tests/scratch_guard.py) with Workspace(torch.device("cpu")), of the
completeness of the GPU table (tests/test_hip_scratch_exact.py) over the project's own Python files, and, where the
library is built, of every scratch sizer: positive and non-decreasing in each size argument, 0 where it documents a
refusal.  Callers size by bounds and reuse a buffer while it is large enough, which is only right for a monotone sizer.

A write into a guard is here an ordinary in-bounds torch write into memory the test owns."""
import itertools
import os
import re

import pytest
import torch

from gradslam_amd import _C
from tests import scratch_guard as sg
from tests import test_hip_scratch_exact as table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ the harness
def test_exact_size_comes_back_and_tensor_goes_through_the_guarded_buffer(monkeypatch):
    with sg.exact_scratch(monkeypatch, 0x7F) as log:
        ws = _C.Workspace(CPU)
        buf = ws.bytes("a", 1000)
        assert buf.numel() == 1000 and buf.dtype == torch.uint8 and bool((buf == 0x7F).all())
        (name, nbytes, outer), = log
        assert (name, nbytes) == ("a", 1000) and outer.numel() == 2 * sg.GUARD + 1000
        assert buf.data_ptr() == outer.data_ptr() + sg.GUARD
        t = ws.tensor("t", (3, 5), torch.float32)
        assert tuple(t.shape) == (3, 5) and t.dtype == torch.float32
        assert sg.requests(log) == [("a", 1000), ("t", 60)]
        assert t.data_ptr() == log[1][2].data_ptr() + sg.GUARD
        t.fill_(1.0)                                   # (the whole of the exact buffer is the caller's)
        buf.fill_(3)
        assert sg.intact(log) == (True, [])
    assert sg.GUARD % 256 == 0 and sg.GUARD == 16 * 4096


def test_reuse_keeps_the_contents_and_growth_is_a_new_logged_buffer(monkeypatch):
    with sg.exact_scratch(monkeypatch, 0xFF) as log:
        ws = _C.Workspace(CPU)
        a = ws.bytes("x", 512)
        a[:4] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
        for n in (512, 100, 0):                        # smaller or equal: the same buffer, not poisoned again
            b = ws.bytes("x", n)
            assert b.data_ptr() == a.data_ptr() and b.numel() == 512 and b[:4].tolist() == [1, 2, 3, 4]
        assert sg.requests(log) == [("x", 512)]
        c = ws.bytes("x", 513)                         # larger: a new buffer, freshly poisoned, logged
        assert c.numel() == 513 and c.data_ptr() != a.data_ptr() and bool((c == 0xFF).all())
        assert sg.requests(log) == [("x", 512), ("x", 513)]
        assert ws.bytes("y", 8).data_ptr() not in (a.data_ptr(), c.data_ptr())
        # the old buffer is still checked
        log[0][2][sg.GUARD + 512 + 9] = 0
        assert sg.intact(log) == (False, [("x", "trailing", 9, 9)])


def test_zero_bytes_yield_a_pointer(monkeypatch):
    with sg.exact_scratch(monkeypatch, 0x00) as log:
        buf = _C.Workspace(CPU).bytes("z", 0)
        assert buf.data_ptr() != 0 and buf.numel() == 1
        assert sg.requests(log) == [("z", 0)]          # (the log keeps the requested size)
        assert log[0][2].numel() == 2 * sg.GUARD + 1 and sg.intact(log) == (True, [])


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x7F])
def test_one_byte_in_either_guard_is_reported_with_its_offset(monkeypatch, fill):
    n = 777
    with sg.exact_scratch(monkeypatch, fill) as log:
        ws = _C.Workspace(CPU)
        ws.bytes("first", 64)
        ws.bytes("second", n)
        outer = log[1][2]
        outer[sg.GUARD + n] = fill ^ 0x01              # the byte a sizer short by one loses
        assert sg.intact(log) == (False, [("second", "trailing", 0, 0)])
        outer[sg.GUARD + n] = fill
        outer[sg.GUARD - 1] = fill ^ 0x80              # the byte just before the scratch
        assert sg.intact(log) == (False, [("second", "leading", -1, -1)])
        outer[0] = fill ^ 0x80                         # first and last touched offsets
        assert sg.intact(log) == (False, [("second", "leading", -sg.GUARD, -1)])
        outer[0] = outer[sg.GUARD - 1] = fill
        outer[-1] = fill ^ 0xFF
        outer[sg.GUARD + n + 5] = fill ^ 0xFF
        log[0][2][sg.GUARD + 64] = fill ^ 0xFF
        assert sg.intact(log) == (False, [("first", "trailing", 0, 0), ("second", "trailing", 5, sg.GUARD - 1)])


def test_a_buffer_outside_the_workspace_is_guarded_the_same_way():
    log = sg.GuardLog(0xFF)
    buf = sg.guarded_buffer(log, "tape", 328, CPU)
    assert buf.numel() == 328 and sg.requests(log) == [("tape", 328)] and sg.intact(log) == (True, [])
    log[0][2][sg.GUARD - 2] = 0
    assert sg.intact(log) == (False, [("tape", "leading", -2, -2)])


def test_instances_and_bytes_are_restored_also_when_the_body_raises(monkeypatch):
    before_bytes = _C.Workspace.bytes
    marker = object()
    _C.Workspace._instances["marker"] = marker
    before = dict(_C.Workspace._instances)          # (with the workspaces of whatever ran earlier in the process)
    try:
        with sg.exact_scratch(monkeypatch, 0x00):
            assert _C.Workspace._instances == {} and _C.Workspace.bytes is not before_bytes
            _C.Workspace._instances["inside"] = _C.Workspace(CPU)
        assert _C.Workspace._instances == before and _C.Workspace.bytes is before_bytes
        with pytest.raises(KeyError):
            with sg.exact_scratch(monkeypatch, 0x00):
                _C.Workspace._instances["inside"] = _C.Workspace(CPU)
                raise KeyError("the body fails")
        assert _C.Workspace._instances == before and _C.Workspace.bytes is before_bytes
        # production's growth rule is back
        assert _C.Workspace(CPU).bytes("a", 1000).numel() == 1000 + 500 + 4096
    finally:
        del _C.Workspace._instances["marker"]


# ------------------------------------------------------------------------------------------ completeness of the GPU table
def workspace_names():
    """every name ops.py and slam/_fastpath.py pass to .bytes( -- and "scratch", the name behind .scratch("""
    names = set()
    for rel in ("gradslam_amd/ops.py", "gradslam_amd/slam/_fastpath.py"):
        with open(os.path.join(REPO, rel)) as f:
            text = f.read()
        found = re.findall(r"\.bytes\(\s*([^,]+),", text)
        for arg in found:
            m = re.match(r"\"([^\"]+)\"(\s*%\s*\w+)?$", arg.strip())
            assert m, "%s: a workspace name this check cannot read: %r" % (rel, arg)
            names.add(m.group(1))
        if re.search(r"\.scratch\(", text):
            names.add("scratch")
    return names


def sizer_exports():
    return {n for n in _C.EXPORTS if n.endswith("_scratch_bytes")}


def test_every_workspace_name_has_a_row():
    names = workspace_names()
    assert {"scratch", "knn_grid", "icp", "icp_bwd", "localize%d", "map_update", "map_update%d", "picp%d"} <= names
    assert names - table.table_names() == set(), "a scratch user without a row in tests/test_hip_scratch_exact.py"
    assert table.table_names() - names == set(), "a row for a workspace name nothing asks for"


def test_every_sizer_export_has_a_row():
    assert len(sizer_exports()) >= 22
    assert sizer_exports() - table.table_sizers() == set(), "a sizer without a row in tests/test_hip_scratch_exact.py"
    assert table.table_sizers() <= set(_C.EXPORTS)


def test_the_completeness_check_fails_when_a_row_is_taken_out(monkeypatch):
    rows = [r for r in table.ROWS if "knn_grid" not in r.names]
    monkeypatch.setattr(table, "ROWS", rows)
    assert workspace_names() - table.table_names() == {"knn_grid"}
    assert sizer_exports() - table.table_sizers() == {"gs_knn1_grid_scratch_bytes"}


def test_row_ids_are_unique_and_every_row_states_names_and_sizers():
    ids = [r.id for r in table.ROWS]
    assert len(ids) == len(set(ids))
    assert all(r.names and r.sizers for r in table.ROWS)


# ------------------------------------------------------------------------------------------ the sizers
ROWS = (0, 1, 1023, 1024, 1025, 70001)
IMAGES = ((1, 1), (5, 7), (17, 31), (37, 53), (257, 257))
# H and W are stepped on their own, over every pair of a height and a width of IMAGES (the images themselves among them):
# a sizer that grows with H W but shrinks with W alone through a per-row term must not pass
HEIGHTS, WIDTHS = tuple(h for h, _ in IMAGES), tuple(w for _, w in IMAGES)
STEPS = (1, 3, 4)
# export: its arguments.  "rows" / "rows2": a row count; "H", "W": a height and a width of IMAGES; "step": a stride or ds of STEPS;
# "views" / "B": 1, 2, 4, 5, 9; "flag": 0, 1
SIZERS = {
    "gs_scratch_bytes": ("rows", "rows2"),
    "gs_knn1_grid_scratch_bytes": ("rows", "rows2"),
    "gs_icp_scratch_bytes": ("rows", "rows2"),
    "gs_icp_backward_scratch_bytes": ("rows", "rows2"),
    "gs_frame_maps_backward_kbar_scratch_bytes": ("H", "W"),
    "gs_global_maps_pose_backward_scratch_bytes": ("H", "W"),
    "gs_update_map_scratch_bytes": ("rows", "H", "W"),
    "gs_localize_scratch_bytes": ("H", "W", "step", "rows"),
    "gs_render_scratch_bytes": ("views", "H", "W"),
    "gs_render_backward_scratch_bytes": ("views", "H", "W", "rows"),
    "gs_prune_scratch_bytes": ("rows",),
    "gs_voxel_keep_scratch_bytes": ("rows",),
    "gs_projective_icp_scratch_bytes": ("H", "W", "step"),
    "gs_projective_icp_scaled_scratch_bytes": ("H", "W", "step"),
    "gs_projective_icp_color_scratch_bytes": ("H", "W", "step"),
    "gs_projective_icp_color_scaled_scratch_bytes": ("H", "W", "step"),
    "gs_projective_icp_color_joint_scaled_scratch_bytes": ("H", "W", "step"),
    "gs_projective_icp_backward_scratch_bytes": ("H", "W", "step", "rows"),
    "gs_projective_icp_ordered_backward_scratch_bytes": ("H", "W", "step", "rows"),
    "gs_projective_icp_ordered_backward_sort_scratch_bytes": ("B", "H", "W", "step"),
    "gs_projective_icp_weighted_backward_scratch_bytes": ("H", "W", "step", "rows", "flag"),
    "gs_picp_outlier_classes_scratch_bytes": ("H", "W"),
    # (the two tape sizers are no *_scratch_bytes exports; they are held the same way)
    "gs_icp_tape_bytes": ("rows", "iters"),
    "gs_projective_icp_tape_bytes": ("iters1",),
}
COUNTS = {"views": (1, 2, 4, 5, 9), "B": (1, 2, 4, 5, 9), "iters": (0, 1, 2, 20), "iters1": (1, 2, 20)}


def test_the_sizer_table_is_complete():
    assert sizer_exports() <= set(SIZERS) and set(SIZERS) <= set(_C.EXPORTS)
    for name, kinds in SIZERS.items():
        assert len(kinds) == len(_C._PROTOS[name]), name


def grid(kinds):
    """[(fixed arguments as a dict kind -> value)] x the axes that grow: every combination of the other arguments, and
    per combination one chain of values per size argument"""
    axes = []
    for k in kinds:
        if k == "H":
            axes.append((k, HEIGHTS))
        elif k == "W":
            axes.append((k, WIDTHS))
        elif k in ("rows", "rows2"):
            axes.append((k, ROWS))
        elif k == "step":
            axes.append((k, STEPS))
        elif k == "flag":
            axes.append((k, (0, 1)))
        elif k in COUNTS:
            axes.append((k, COUNTS[k]))
    return axes


def call(lib, name, kinds, values):
    return int(getattr(lib, name)(*[values[k] for k in kinds]))


@pytest.mark.parametrize("name", sorted(SIZERS))
def test_sizer_is_positive_and_non_decreasing_in_each_size_argument(name):
    lib = _C.lib()
    kinds = SIZERS[name]
    axes = grid(kinds)
    growing = [a for a, _ in axes if a not in ("step", "flag")]      # (a stride thins the lattice: not a size)
    for combo in itertools.product(*[v for _, v in axes]):
        values = dict(zip([a for a, _ in axes], combo))
        here = call(lib, name, kinds, values)
        assert here > 0, (name, values, here)
        for a in growing:
            chain = dict(axes)[a]
            i = chain.index(values[a])
            if i + 1 < len(chain):
                more = call(lib, name, kinds, dict(values, **{a: chain[i + 1]}))
                assert more >= here, (name, "shrinks when %s grows" % a, values, here, chain[i + 1], more)


# the refusals the header documents: "Both return 0 on bad arguments (the second also when min(B, 8) nslots >= 2^31)" for
# the ordered backward's two sizers, "0 for bad sizes" for the joint scaled one
@pytest.mark.parametrize("name,bad", [
    ("gs_projective_icp_ordered_backward_scratch_bytes", [(0, 7, 1, 10), (5, 0, 1, 10), (5, 7, 0, 10), (5, 7, 1, -1),
                                                          (-5, 7, 1, 10), (65536, 32768, 1, 10)]),
    ("gs_projective_icp_ordered_backward_sort_scratch_bytes", [(0, 5, 7, 1), (1, 0, 7, 1), (1, 5, 0, 1), (1, 5, 7, 0),
                                                               (-1, 5, 7, 1), (1, 65536, 32768, 1), (2, 32768, 32768, 1),
                                                               (9, 32768, 32768, 2)]),
    ("gs_projective_icp_color_joint_scaled_scratch_bytes", [(0, 7, 1), (5, 0, 1), (5, 7, 0), (5, -7, 1),
                                                            (65536, 32768, 1)]),
])
def test_sizer_returns_zero_where_it_documents_a_refusal(name, bad):
    lib = _C.lib()
    for args in bad:
        assert getattr(lib, name)(*args) == 0, (name, args)
    # ... and just inside: one launch group of 8 lattices below 2^31 pairs
    if name.endswith("sort_scratch_bytes"):
        assert lib.gs_projective_icp_ordered_backward_sort_scratch_bytes(1, 32768, 32768, 1) > 0
        assert lib.gs_projective_icp_ordered_backward_sort_scratch_bytes(9, 32768, 32768, 3) > 0
