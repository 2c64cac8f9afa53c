"""CPU-side checks of the measurement plumbing: the synthetic workload generator, the profile-summary parser and the
committed bench lines (the numbers themselves are measured on the MI355X; here only their consistency)."""
import glob
import json
import os

import numpy as np

import bench
from gradslam_amd.datasets import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camera_path_turns_back_and_early_frames_are_unchanged():
    # the goldens were recorded on the first frames of the one-way path: identity there
    for s in range(0, synthetic.PATH_TURN + 1, 7):
        assert synthetic.path_parameter(s) == s
    assert synthetic.path_parameter(synthetic.PATH_TURN + 10) == synthetic.PATH_TURN - 10
    assert synthetic.path_parameter(2 * synthetic.PATH_TURN) == 0
    assert np.array_equal(synthetic.gt_pose(2 * synthetic.PATH_TURN + 3), synthetic.gt_pose(3))
    yaw = max(abs(np.arctan2(synthetic.gt_pose(s)[0, 2], synthetic.gt_pose(s)[0, 0])) for s in range(0, 1000, 13))
    assert yaw <= 0.3 + 1e-6


def test_chunked_generation_is_a_function_of_the_frame_index():
    """bench.make_sequences builds long sequences from chunks generated in parallel: geometry (depth before the
    holes, poses) of a frame must not depend on the chunking."""
    a = synthetic.make_sequence(4, 24, 32, seed=2, first=8)
    b = synthetic.make_sequence(2, 24, 32, seed=2, first=10)
    assert np.array_equal(a["poses"][2:], b["poses"])
    both = (a["depths"][2:] > 0) & (b["depths"] > 0)    # the hole streams differ per chunk
    assert both.mean() > 0.8 and np.array_equal(a["depths"][2:][both], b["depths"][both])


def test_sequences_generated_in_process_under_a_profiler(monkeypatch):
    monkeypatch.setenv("ROCPROFILER_LIBRARY_CTOR", "1")
    seqs = bench.make_sequences([0, 1], 2, 24, 32)
    assert len(seqs) == 2 and seqs[0]["depths"].shape == (2, 24, 32, 1)
    ref = synthetic.make_sequence(2, 24, 32, seed=1)
    assert np.array_equal(seqs[1]["depths"], ref["depths"])


def test_pmc_summary_parser_and_committed_bench_lines():
    traffic, src = bench.pmc_traffic("gs_icp_half_batch_kernel")
    assert src is not None and src["file"].startswith("profiles/") and 1e6 < traffic < 1e9
    assert src["command"] and "bench.py" in src["command"]          # the run the counters came from, on record
    lines = sorted(glob.glob(os.path.join(REPO, "profiles", "r02_*_bench_line.json")))
    assert lines
    for path in lines:
        d = json.load(open(path))
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
            assert k in d, (path, k)
        assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
        # value = sequences * steps / time
        seqs = d["config"]["sequences_total"]
        assert abs(d["value"] - seqs * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        r = d.get("roofline")
        if r:
            assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
            if r.get("traffic") is not None:
                assert r["alg_le_traffic"] == (r["alg_bytes_per_launch"] <= r["traffic"])


def test_dump_outputs_is_seeded_bounded_and_complete(tmp_path):
    """bench.py --dump-outputs: the poses of the last step, the map sizes and a fixed seeded sample of every map, in
    float32 / float64, identical for identical results and within the size bound whatever the maps' sizes."""
    import torch
    from gradslam_amd.structures.pointclouds import Pointclouds
    rng = np.random.default_rng(0)
    small, big = 1000, bench.DUMP_MAX_ROWS   # one map below the per-sequence share, one above it
    lists = {k: [torch.from_numpy(rng.random((n, w), dtype=np.float32)) for n in (small, big)]
             for k, w in (("points", 3), ("normals", 3), ("colors", 3), ("features", 1))}
    maps = Pointclouds(**lists)
    poses = torch.from_numpy(rng.random((2, 7, 4, 4), dtype=np.float32))
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), poses, maps)
        outs.append({os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(str(tmp_path / d / "*.npy")))})
    a, b = outs
    assert sorted(a) == ["map_colors", "map_counts", "map_features", "map_normals", "map_points", "map_rows", "poses",
                         "trajectory"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) < 64 << 20
    assert np.array_equal(a["poses"], poses[:, -1].numpy()) and np.array_equal(a["trajectory"], poses.numpy())
    assert a["map_counts"].tolist() == [small, big]
    seq, row = a["map_rows"][:, 0].astype(np.int64), a["map_rows"][:, 1].astype(np.int64)
    share = bench.DUMP_MAX_ROWS // 2
    assert (seq == 0).sum() == small and (seq == 1).sum() == share and len(np.unique(row[seq == 1])) == share
    for k in ("points", "normals", "colors", "features"):
        for s in (0, 1):
            assert np.array_equal(a["map_" + k][seq == s], lists[k][s].numpy()[row[seq == s]]), (k, s)


def test_device_generator_matches_the_host_scene_and_is_seeded():
    """A long plain bench run generates its frames on the device (bench.make_sequences_on_device; run here on the CPU
    device): the scene and camera path of synthetic.make_sequence (the same depth wherever neither has a hole, the
    same poses, the first pose alone given), 5 % holes, colours in [0, 255), identical for identical arguments."""
    import torch
    import gradslam_amd as gs
    seeds, L, H, W = [0, 3], 70, 24, 32
    fr, seqs = bench.make_sequences_on_device(gs, seeds, L, H, W, torch.device("cpu"))
    fr2, _ = bench.make_sequences_on_device(gs, seeds, L, H, W, torch.device("cpu"))
    assert torch.equal(fr.depth_image, fr2.depth_image) and torch.equal(fr.rgb_image, fr2.rgb_image)
    d, c = fr.depth_image.numpy(), fr.rgb_image.numpy()
    assert d.shape == (2, L, H, W, 1) and c.shape == (2, L, H, W, 3) and 0.0 <= c.min() and c.max() < 255.0
    assert torch.equal(fr.poses, fr.poses[:, :1].expand(2, L, 4, 4))
    for b, sd in enumerate(seeds):
        ref = synthetic.make_sequence(L, H, W, seed=sd)
        assert np.array_equal(seqs[b]["poses"], ref["poses"]) and np.array_equal(fr.poses[b, 0].numpy(), ref["poses"][0])
        assert np.array_equal(fr.intrinsics[b, 0].numpy(), ref["intrinsics"][0])
        both = (d[b] > 0) & (ref["depths"] > 0)
        assert 0.85 < both.mean() and 0.04 < (d[b] == 0).mean() < 0.06
        assert np.abs(d[b][both] / ref["depths"][both] - 1.0).max() < 1e-6
