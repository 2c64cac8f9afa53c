"""The host layer of the projective ICP makes the library calls it made before it was restructured: the call log of the
tree (tests/picp_call_log.py) equals tests/golden/picp_call_log.txt, recorded at the commit before, apart from one named
difference; and the one routing function states the table of entries literally.  No GPU: nothing is launched."""
import itertools
import os
import re

import pytest

from gradslam_amd import _C, ops
from tests import picp_call_log

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picp_call_log.txt")
ENDS = ("CALL ", "RET ", "RAISED ", "== ", "GRADS ")                 # a line of these ends a segment of the log
FORWARD_SCRATCH = re.compile(r"ws picp\d+ \d+")                      # (fullmatch: not picp_bwd<b>, not picp_bwd_sort)
BACKWARD_CALL = re.compile(r"CALL gs_projective_icp_(\w+_)?backward_batch_f32 ")


def without_the_backwards_forward_scratch(text):
    """The log without the one thing that was dropped on purpose: projective_icp_backward_batch used to ask the workspace
    for the forward's scratch (`ws picp<b> <bytes>`), which it never handed to the library.  Exactly these lines go: a
    forward-scratch request whose segment (the lines up to the next CALL / RET / RAISED / == / GRADS line) ends in the
    call of a backward export, or in a refusal of the backward after its descriptors were built."""
    lines, out, pending, dropped = text.split("\n"), [], [], 0
    for line in lines:
        if not line.startswith(ENDS):
            pending.append(line)
            continue
        backward = BACKWARD_CALL.match(line) or (line.startswith("RAISED ") and ": projective_icp_backward: " in line)
        kept = [p for p in pending if not (backward and FORWARD_SCRATCH.fullmatch(p))]
        dropped += len(pending) - len(kept)
        out += kept + [line]
        pending = []
    return "\n".join(out + pending), dropped


@pytest.fixture(scope="module")
def logs():
    with open(GOLDEN) as f:
        return f.read(), picp_call_log.log()


def test_the_tree_makes_the_calls_of_the_golden_log(logs):
    golden, got = logs
    want, dropped = without_the_backwards_forward_scratch(golden)
    # one per sequence of every backward, no more: as many as the backward's own scratch requests, plus those of the
    # two refusals of the grid that come between the descriptors and the backward's scratch
    early = sum(golden.count("RAISED ValueError: projective_icp_backward: " + m) for m in ("tapes must be", "want_maps"))
    assert dropped == len(re.findall(r"^ws picp_bwd\d+ ", golden, re.M)) + picp_call_log.B * early and early == 2
    assert without_the_backwards_forward_scratch(got) == (got, 0)             # the tree no longer asks for it
    if got != want:
        a, b = want.split("\n"), got.split("\n")
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        case = next(line for line in reversed(a[:first + 1]) if line.startswith("== "))
        pytest.fail("the call log differs from the golden one at line %d, in case %r:\n  golden: %s\n  tree:   %s"
                    % (first + 1, case, a[first] if first < len(a) else "<end>", b[first] if first < len(b) else "<end>"))


def test_the_log_reaches_every_projective_export_and_stays_small(logs):
    golden, _ = logs
    called = set(re.findall(r"^CALL (\w+)", golden, re.M))
    entries = {n for n in _C.EXPORTS if n.startswith("gs_projective_icp_") and n.endswith("_f32")}
    assert entries and entries <= called
    for key in ("ws picp0 ", "ws picp_bwd0 ", "ws picp_bwd_sort "):
        assert key in golden
    assert os.path.getsize(GOLDEN) < 200 * 1024


# ---------------------------------------------------------------------------------------- the routing table, literally
# per family: the rungs in order, (condition, export); the first that holds serves the call
def _rungs(family, o, weights, tape, ordered, tables):
    k, ck, d, cd = o.huber_k > 0, o.color_huber_k > 0, o.huber_delta > 0, o.color_huber_delta > 0
    return {
        "batch": [(weights, "weighted_batch"), (k, "scaled_batch"), (d, "robust_batch"), (tape, "tape_batch"),
                  (True, "batch")],
        "rows": [(weights, "weighted_rows"), (k, "scaled_rows"), (d or tables, "robust_rows"), (True, "rows")],
        "color_batch": [(weights, "color_weighted_batch"), (ck, "color_joint_scaled_batch"), (k, "color_scaled_batch"),
                        (d or cd, "color_robust_batch"), (True, "color_batch")],
        "color_rows": [(weights, "color_weighted_rows"), (k or ck, "color_joint_scaled_rows"),
                       (d or cd or tables, "color_robust_rows"), (True, "color_rows")],
        "backward": [(weights, "weighted_backward"), (ordered, "ordered_backward"), (k, "scaled_backward"),
                     (d, "robust_backward"), (True, "backward")],
    }[family]


def _sizer(family, o, weights, ordered, tables):
    k, ck = o.huber_k > 0, o.color_huber_k > 0
    if family in ("batch", "rows"):
        return "scaled" if k else "plain"
    if family == "color_batch":
        return "joint_scaled" if ck or (weights and k) else "color_scaled" if k else "color"
    if family == "color_rows":
        return "joint_scaled" if k or ck else "color"
    return "weighted_backward" if tables else "ordered_backward" if ordered else "backward"


def test_the_route_is_the_table_of_entries():
    families = ("batch", "rows", "color_batch", "color_rows", "backward")
    seen = set()
    for family, d, k, cd, ck, weights, tape, ordered, tables in itertools.product(
            families, (0.0, 0.05), (0.0, 1.345), (0.0, 0.1), (0.0, 1.345), *[(False, True)] * 4):
        colour = family.startswith("color")
        if not colour and (cd or ck):
            continue
        # what no entry takes: a tape outside the batch family, the ordered mode outside the backward, the per-slot
        # output outside the rows families and the weighted backward
        impossible = (tape and family != "batch") or (ordered and family != "backward") or \
            (tables and not (family.endswith("rows") or (family == "backward" and weights)))
        if impossible:
            with pytest.raises(ValueError, match="no projective ICP entry"):
                ops._picp_route(family, ops.PicpOptions(huber_delta=d, huber_k=k), weights=weights, tape=tape,
                                ordered=ordered, tables=tables)
            continue
        o = ops.PicpOptions(huber_delta=d, huber_k=k, color_weight=0.3 if colour else 0.0, color_huber_delta=cd,
                            color_huber_k=ck)
        export = next(name for cond, name in _rungs(family, o, weights, tape, ordered, tables) if cond)
        got = ops._picp_route(family, o, weights=weights, tape=tape, ordered=ordered, tables=tables)
        assert got == (export, _sizer(family, o, weights, ordered, tables)), (family, o, weights, tape, ordered, tables)
        seen.add(got[0])
        name = "gs_projective_icp_%s_f32" % export if family != "backward" else "gs_projective_icp_%s_batch_f32" % export
        assert name in _C.EXPORTS and ops._PICP_SIZERS[got[1]] in _C.EXPORTS
    # every entry point of the library has a rung, and every rung an entry point
    assert {"gs_projective_icp_%s%s_f32" % (e, "_batch" if e.endswith("backward") else "") for e in seen} == \
        {n for n in _C.EXPORTS if n.startswith("gs_projective_icp_") and n.endswith("_f32")}
    with pytest.raises(ValueError):
        ops._picp_route("colour", ops.PicpOptions())


def test_the_options_are_validated_once_in_the_order_written():
    o = ops._picp_options("who", geometry=(2, 3, 1e-8, 0.1, 60.0), huber_delta=1, flags=("flag",), flag=True,
                          deterministic=None)
    assert o == ops.PicpOptions(stride=2, numiters=3, damp=1e-8, dist_th=0.1, dot_th=o.dot_th, huber_delta=1.0)
    assert abs(o.dot_th - 0.5) < 1e-12 and isinstance(o.huber_delta, float)
    with pytest.raises(TypeError, match="who: huber_k must be of type float or int"):
        ops._picp_options("who", huber_k=True, huber_delta=-1)            # the first keyword is refused first
    with pytest.raises(ValueError, match=r"who: huber_delta \(-1\) must be finite and not negative"):
        ops._picp_options("who", huber_delta=-1, huber_k=True)
    with pytest.raises(TypeError, match="who: flag must be of type bool"):
        ops._picp_options("who", flags=("flag",), flag=1)
    with pytest.raises(TypeError, match="'huber_delt' is neither an option nor one of the flags"):
        ops._picp_options("who", huber_delt=0.05)                            # a misspelt option is not taken for a flag
    with pytest.raises(ValueError, match="projective_icp: stride"):          # (_picp_args names the solve, whoever asks)
        ops._picp_options("who", geometry=(0, 3, 1e-8, 0.1, 60.0))
    with pytest.raises(ValueError, match="projective_icp_color: color_weight"):
        ops._picp_options("who", color_weight=-1)
    with pytest.raises(ValueError, match="who: color_huber_k > 0 needs color_weight > 0"):
        ops._picp_options("who", color_weight=0, color_huber_k=1.0)
    base = ops._picp_options("who", color_weight=0)                          # (the rule binds within one call only)
    assert ops._picp_options("who", base, color_huber_k=1.0).color_huber_k == 1.0
