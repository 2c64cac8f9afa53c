"""GPU: every engine switch of the ICP solve against the ORACLE, not against another HIP run.

The solve (csrc/gs_icp_loop.hip, gs_knn.h) has runtime switches that pick other kernels or branches: candidate lists,
wide lists, binned normals, weak-list room, the brute-force search.  None may
change a result, and an A/B pair of two HIP runs cannot see a bug both of its sides share (a cube scan, the block-wide
pass, the partial last row unit of 96 points).  So every (setting, scene) below runs in a fresh process -- the switches
are read into statics once per process -- and is held to the oracle's record of the scene
(tests/golden/engine_<scene>_oracle.npz, oracle/make_golden_engine.py): poses bit for bit, surfel counts equal, sampled
map rows within 1e-5 (as tests/test_hip_batch.py::test_pointfusion_640x480_vs_oracle), float64 point sums within what
that bound allows.  A setting whose path could be skipped without a word also asserts that it ran (the witness).

Scenes: bench8 (the benchmark's shard, 8 x 480x640), hard3 (frames 85..88: cube scans, wide lists, block passes),
ragged2 (67x131: 561 source points, the last row unit partial), weak1 (9 frames: weak lists at frame 8)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NUMITERS = 20   # PointFusion(odom="gradicp") default: the solve's 2 x 20 half-iterations

# One child per (setting, scene).  mode "step": PointFusion.step (the one-call frame loop, gs_pointfusion_step_batch_f32);
# mode "plugin": the same SLAM loop with the solve routed through the generic provider path (ops.icp per sequence,
# gs_icp_f32), the only path GRADSLAM_HIP_KNN reaches.
_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.datasets.synthetic import make_sequence
from gradslam_amd.odometry import GradICPOdometryProvider
out, fixture, mode = sys.argv[1], sys.argv[2], sys.argv[3]
g = np.load(fixture)
H, W, L, first = int(g["H"]), int(g["W"]), int(g["L"]), int(g["first"])
seeds = [int(x) for x in g["seeds"]]
B = len(seeds)
seqs = [make_sequence(L, H, W, seed=sd, first=first) for sd in seeds]
st = lambda k: torch.from_numpy(np.stack([s[k] for s in seqs])).cuda()
poses = st("poses"); poses[:, 1:] = poses[:, :1]
frames = gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)
slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
if mode == "plugin":
    class Plugin(GradICPOdometryProvider):   # (not one of the built-in types: the fast paths step aside)
        pass
    slam.odomprov = Plugin()
pc, prev = gs.Pointclouds(device="cuda"), None
rec, counts, sums, abss, lstats, sstats = [], [], [], [], [], []
for i in range(L):
    live = frames[:, i]
    pc, p = slam.step(pc, live, prev, inplace=True)
    prev = live
    rec.append(p[:, 0].cpu().numpy())
    counts.append([int(x.shape[0]) for x in pc.points_list])
    sums.append([x.double().sum(0).cpu().numpy() for x in pc.points_list])
    abss.append([float(x.double().abs().sum()) for x in pc.points_list])
    if i >= 1 and mode == "step":
        cap = [pc._buf["points"][b].shape[0] for b in range(B)]
        lstats.append([ops.localize_list_stats(torch.device("cuda", 0), b, H, W, 4, cap[b]) for b in range(B)])
        sstats.append([[ops.localize_solve_stats(torch.device("cuda", 0), b, H, W, 4, cap[b])["weak"]] for b in range(B)])
idx = torch.from_numpy(g["sample_idx"].astype(np.int64)).cuda()
sample = np.stack([pc.points_list[b][idx[b]].cpu().numpy() for b in range(B)])
np.savez(out, poses=np.stack(rec).transpose(1, 0, 2, 3), counts=np.array(counts).T, sums=np.stack([np.stack(s) for s in sums]).transpose(1, 0, 2),
         abs_sums=np.array(abss).T, sample=sample, lstats=np.array(lstats), sstats=np.array(sstats, np.int64))
"""
SSTAT = ("weak",)   # (what the child records of ops.localize_solve_stats)

SETTINGS = {
    "default": ({}, "step"),
    "lists0": ({"GRADSLAM_HIP_ICP_LISTS": "0"}, "step"),
    "wide0": ({"GRADSLAM_HIP_ICP_WIDE": "0"}, "step"),
    "binned0": ({"GRADSLAM_HIP_ICP_BINNED_NORMALS": "0"}, "step"),
    "weak008": ({"GRADSLAM_HIP_ICP_WEAK_ROOM": "0.08"}, "step"),
    "brute": ({"GRADSLAM_HIP_KNN": "brute"}, "plugin"),
}
_cache = {}


def _child_env(extra):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("GRADSLAM_HIP_ICP_") or k.startswith("GRADSLAM_HIP_KNN"):
            env.pop(k)
    env.update(extra)
    return env


def _run(setting, scene, tmp_path_factory):
    key = (setting, scene)
    if key not in _cache:
        extra, mode = SETTINGS[setting]
        out = str(tmp_path_factory.mktemp("engine") / ("%s_%s.npz" % key))
        subprocess.run([sys.executable, "-c", _CHILD % REPO, out, _fixture_path(scene), mode], check=True, timeout=900,
                       env=_child_env(extra))
        _cache[key] = dict(np.load(out))
    return _cache[key]


def _fixture_path(scene):
    return os.path.join(GOLDEN, "engine_%s_oracle.npz" % scene)


def _assert_oracle(setting, scene, r):
    """poses bit for bit, counts equal, sampled rows within 1e-5, point sums within the sum of that bound"""
    g = np.load(_fixture_path(scene))
    B, L = g["poses"].shape[:2]
    assert r["poses"].shape == (B, L, 4, 4)
    bound = 1e-5 * (g["counts"] + r["abs_sums"])          # (B, L): |sum of rows within 1e-5 + 1e-5 |x||
    dsum = np.abs(r["sums"] - g["sum_points"]).max(axis=2)
    rec_dir = os.environ.get("GRADSLAM_TEST_RECORD")
    if rec_dir:   # (written before the asserts: a failing run leaves its numbers)
        ss = r["sstats"]
        with open(os.path.join(rec_dir, "engine_%s_%s.json" % (setting, scene)), "w") as fh:
            json.dump({"poses_bit_exact": bool(np.array_equal(r["poses"].view(np.int32), g["poses"].view(np.int32))),
                       "pose_max_abs_diff": float(np.abs(r["poses"] - g["poses"]).max()),
                       "counts_equal": bool(np.array_equal(r["counts"], g["counts"])),
                       "sample_rows_bit_exact": bool(np.array_equal(r["sample"].view(np.int32), g["sample_points"].view(np.int32))),
                       "sample_rows_max_abs_diff": float(np.abs(r["sample"] - g["sample_points"]).max()),
                       "point_sum_max_abs_diff": float(dsum.max()),
                       "solve_stats": ss.tolist(),
                       "weak_lists": int(ss[..., SSTAT.index("weak")].sum()) if ss.size else 0}, fh)
    for b in range(B):
        same = r["poses"][b].view(np.int32) == g["poses"][b].view(np.int32)
        assert same.all(), (setting, scene, b, np.abs(r["poses"][b] - g["poses"][b]).reshape(L, -1).max(1))
    assert np.array_equal(r["counts"], g["counts"]), (setting, scene, r["counts"], g["counts"])
    np.testing.assert_allclose(r["sample"], g["sample_points"], rtol=1e-5, atol=1e-5, err_msg="%s %s" % (setting, scene))
    assert (dsum <= bound).all(), (setting, scene, dsum, bound)


def _stat(r, name):
    return r["sstats"][..., SSTAT.index(name)]               # (frames - 1, B)


@pytest.mark.parametrize("scene", ["bench8", "hard3", "ragged2", "weak1"])
def test_default_engine_matches_oracle(tmp_path_factory, scene):
    """The anchor: the default engine (ordinary + wide candidate lists, binned normals, launch per half-iteration) on every
    scene.  No weak list is counted without GRADSLAM_HIP_ICP_WEAK_ROOM."""
    r = _run("default", scene, tmp_path_factory)
    _assert_oracle("default", scene, r)
    assert not _stat(r, "weak").any()
    if scene == "hard3":   # the scene has points without an ordinary list (what the wide lists, cubes and block passes serve)
        assert r["lstats"][:, :, 2, 4:40].sum() > 0


@pytest.mark.parametrize("scene", ["hard3", "ragged2"])
def test_without_candidate_lists_matches_oracle(tmp_path_factory, scene):
    """GRADSLAM_HIP_ICP_LISTS=0: every half-iteration searches the grid; witness: the list counters stay zero."""
    r = _run("lists0", scene, tmp_path_factory)
    _assert_oracle("lists0", scene, r)
    assert not r["lstats"].any()


def test_without_wide_lists_matches_oracle(tmp_path_factory):
    """GRADSLAM_HIP_ICP_WIDE=0 on the hard frames: the hard points go through the cube scans and block passes every time.
    Witness, as in tests/test_hip_batch.py::test_wide_lists_of_hard_queries_leave_results_identical: the default run has
    points without an ordinary list (served by wide lists), and the list counters of the two runs differ."""
    r = _run("wide0", "hard3", tmp_path_factory)
    _assert_oracle("wide0", "hard3", r)
    d = _run("default", "hard3", tmp_path_factory)
    assert d["lstats"][:, :, 2, 4:40].sum() > 0
    assert not np.array_equal(r["lstats"], d["lstats"])


@pytest.mark.parametrize("scene", ["bench8", "ragged2"])
def test_gathered_normals_match_oracle(tmp_path_factory, scene):
    """GRADSLAM_HIP_ICP_BINNED_NORMALS=0: the matches' normals gathered from the map instead of the binned copy.  No witness
    needed: a host branch with no fallback (the grid build is given no normals)."""
    r = _run("binned0", scene, tmp_path_factory)
    _assert_oracle("binned0", scene, r)


@pytest.mark.parametrize("scene", ["weak1", "bench8"])
def test_weak_list_room_matches_oracle(tmp_path_factory, scene):
    """GRADSLAM_HIP_ICP_WEAK_ROOM=0.08 (DESIGN.md's best bench setting): lists with too little room are re-made by the
    cube scans of the list-building launch.  Witness: some solve flagged weak lists."""
    r = _run("weak008", scene, tmp_path_factory)
    _assert_oracle("weak008", scene, r)
    assert _stat(r, "weak").sum() > 0


@pytest.mark.parametrize("scene", ["ragged2", "weak1"])
def test_brute_force_search_matches_oracle(tmp_path_factory, scene):
    """GRADSLAM_HIP_KNN=brute: the brute-force nearest-neighbour engine of gs_icp_f32.  That switch acts on the generic
    solve only (the one-call frame loop always bins its targets), so this run routes the solve through a provider of
    its own type, which the fast paths step aside for.  No witness needed: a host branch with no fallback."""
    r = _run("brute", scene, tmp_path_factory)
    _assert_oracle("brute", scene, r)
