"""Pins the C oracle (oracle/gs_oracle.c) to the REAL reference on the constructed edge scenes of the map update
(tests/golden/fusion_edges.npz, recorded by oracle/make_golden_fusion_edges.py): frame borders and rounding ties of the
projection, pairs on the similarity thresholds, bit-identical keys, the merge's corner values, the ordered append and
batches in which some sequences have no match.  Tables, masks and counts bit-exact; fused values bit-exact (the oracle is
fed the reference's alpha and global maps), the sign of zero included.  CPU only."""
import numpy as np
import pytest

from oracle import fusion_edges as fe

SCENES = ["borders", "borders_kzero", "borders_perm", "general_ragged", "general_dense", "thresholds", "thresholds_nodepth",
          "ties", "ties_one_mark", "ties_no_mark", "merge", "merge_nomatch", "append_all_new", "append_none_new",
          "append_last_tile", "append_first_only", "append_last_only", "batch9", "batch9_late", "batch2_one_empty_table",
          "tiny_1x1", "tiny_2x2"]


def test_the_file_holds_exactly_these_scenes(golden):
    assert fe.scene_names(golden("fusion_edges")) == SCENES


@pytest.mark.parametrize("name", SCENES)
def test_oracle_reproduces_the_reference(golden, name):
    g = golden("fusion_edges")
    sc = fe.load_scene(g, name)
    tabs = fe.oracle_scene(sc)
    fe.assert_oracle_is_reference(sc, tabs)
    if name + "/expect_best" in g.files:   # the winner of every pixel, written down by hand
        assert np.array_equal(tabs[0]["best"], g[name + "/expect_best"])


def test_batch_scenes_are_what_they_claim(golden):
    """batch9_late: only the last sequence (second chunk of 8) has a match, and the first chunk's rows are still rewritten
    as (cc * x) * (1 / cc), which is not the identity in float32; merge_nomatch: no match in the call, bits untouched."""
    g = golden("fusion_edges")
    sc = fe.load_scene(g, "batch9_late")
    assert [s["unique"].shape[0] > 0 for s in sc["seqs"]] == [False] * 8 + [True]
    assert any(not np.array_equal(s["fP"][: s["P"].shape[0]], s["P"]) for s in sc["seqs"][:8])
    s = fe.load_scene(g, "merge_nomatch")["seqs"][0]
    for k in "PNCF":
        fe.same_bits(s["f" + k][: s[k].shape[0]], s[k], "merge_nomatch " + k)
    sc = fe.load_scene(g, "batch2_one_empty_table")
    assert [s["unique"].shape[0] > 0 for s in sc["seqs"]] == [False, True]
