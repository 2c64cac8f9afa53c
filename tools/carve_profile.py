"""Free-space carving: what one carve pass costs and what carving costs the frame loop (needs the MI355X; fails
without one).

    python tools/carve_profile.py [--out FILE] [--only carve|slam] [--steps K [K ...]]

1. Time of one carve pass (gs_free_space_dc_f32, without the compaction that follows it in Pointclouds.carve_).  The
   maps are the ones the benchmark builds: B = 8 sequences of 640x480 stepped for 40 frames with PointFusion, their
   counts left on the device; the views are the last L frames of each sequence under the poses the steps recovered,
   L = 1 and L = 8.
     new       one ops.free_space_batch call (window 1): all B maps, all L views, one launch.
     baseline  the torch composition of calls the package had before: per map and view ops.project_map (the same
               projection, HIP), the camera-frame depth by a torch matmul, a gather of the (2 window + 1)^2 depths
               with clamped indices, compare and reduce.  Its z comes from a differently ordered sum, so the two are
               compared as counts of differing rows (reported; expected to be a handful of rows at the margin), not
               bit for bit.
   Timing: device events around `reps` back-to-back calls that end in a synchronise, the two variants alternating in
   one process after a warm-up of each shape; median / min / max over the rounds.  Bytes the algorithm needs per map of
   n rows: 12 n (points) + 4 n L (one depth gather per row and view, an upper bound: rows outside a frame gather
   nothing) + 5 n (both outputs); the window is read only for rows whose centre pixel violates.  The share of the HBM
   peak that these bytes over the measured time come to is bytes-bound (the pass does no arithmetic to speak of); the
   gathers are 4-byte reads scattered over cache lines, so the share says how far a gather-bound pass sits from a
   streaming one.

2. What carving costs.  The K-step B = 8 run at 640x480 (K = 20 after 5 warm-up frames as bench.py, K = 200 after 30;
   frames generated on the device as bench.py does), without and with PointFusion(carve_margin=0.05), the run without
   repeated for the spread of the same code.  The scene is static: the carve removes next to nothing, so the difference
   is the cost of the pass and of the compaction that follows it on every step.  Reported: frames/s, step time per
   quartile, final rows per sequence, rows removed, ATE against ground truth."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
MARGIN, WINDOW = 0.05, 1


def time_pair(torch, fa, fb, reps, rounds):
    res = {"a": [], "b": []}
    for _ in range(rounds):
        for key, fn in (("a", fa), ("b", fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[key].append(e0.elapsed_time(e1) / reps)
    return res["a"], res["b"]


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def baseline(torch, ops, maps, depth, poses, K, H, W):
    """violations per map through existing calls: HIP projection, then torch for z, the gathers and the compare"""
    out = []
    margin = torch.tensor(MARGIN, dtype=torch.float32, device=depth.device)
    for b, m in enumerate(maps):
        P, n, n_dev = m[0], m[4], m[5]
        viol = torch.zeros(n, dtype=torch.int32, device=P.device)
        for l in range(depth.shape[1]):
            pix = ops.project_map(P[:n], poses[b, l], K[b], H, W, n_dev=n_dev).long()
            T = poses[b, l]
            z = (P[:n] - T[:3, 3]) @ T[:3, 2]
            inside = pix >= 0
            p = pix.clamp(min=0)
            h, w = p // W, p % W
            D = depth[b, l]
            ok = inside & (D[h, w] > 0)
            for dh in range(-WINDOW, WINDOW + 1):
                for dw in range(-WINDOW, WINDOW + 1):
                    hh, ww = h + dh, w + dw
                    within = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
                    d = D[hh.clamp(0, H - 1), ww.clamp(0, W - 1)]
                    ok &= ~(within & (d > 0)) | ((d - z) > margin)
            viol += ok.to(torch.int32)
        out.append(viol)
    return out


def carve_times(torch, gs, ops, reps=5, rounds=7):
    import bench
    B, steps, H, W = 8, 40, 480, 640
    device = torch.device("cuda")
    frames, _ = bench.make_sequences_on_device(gs, list(range(B)), steps, H, W, device)
    slam = gs.slam.PointFusion(odom="gradicp", device=device)
    r = bench.timed_steps(gs, slam, frames, 5, steps - 5, device, lambda: torch.cuda.synchronize(device))
    pc, rec_poses = r["pc"], r["poses"]
    counts = pc._tighten_counts()
    maps = []
    for b in range(B):
        bound, n_dev = pc._count_of(b)
        maps.append((pc._buf["points"][b], None, None, None, bound, n_dev))
    K = frames.intrinsics[:, 0].contiguous()
    out = []
    for L in (1, 8):
        depth = frames.depth_image[:, steps - L:, :, :, 0].contiguous()
        poses = rec_poses[:, steps - L:].contiguous()
        new = lambda: ops.free_space_batch(maps, depth, poses, K, margin=MARGIN, window=WINDOW)       # noqa: E731
        old = lambda: baseline(torch, ops, maps, depth, poses, K, H, W)                               # noqa: E731
        a, o = new(), old()
        differ = [int((a.violations[b][:counts[b]] != o[b][:counts[b]]).sum()) for b in range(B)]
        violating = [int((a.violations[b][:counts[b]] > 0).sum()) for b in range(B)]
        del a, o
        for _ in range(2):
            new(), old()
        t_new, t_old = time_pair(torch, new, old, reps, rounds)
        alg = sum(12 * n + 4 * n * L + 5 * n for n in counts)
        s_new, s_old = stats(t_new), stats(t_old)
        rec = {"B": B, "views": L, "window": WINDOW, "rows_per_map": counts, "rows_violating": violating,
               "rows_on_which_the_baseline_differs": differ, "new": s_new, "baseline": s_old,
               "speedup_median": s_old["median_ms"] / s_new["median_ms"], "algorithmic_bytes": alg,
               "new_share_of_hbm_peak_bytes_bound": alg / (s_new["median_ms"] * 1e-3) / HBM_PEAK}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def slam_runs(torch, gs, steps, Wm):
    import bench
    from gradslam_amd.metrics import ate_rmse
    B = 8
    device = torch.device("cuda")
    frames, seqs = bench.make_sequences_on_device(gs, list(range(B)), Wm + steps, 480, 640, device)
    gt = np.stack([s["poses"] for s in seqs])

    def run(**kw):
        slam = gs.slam.PointFusion(odom="gradicp", device=device, **kw)
        r = bench.timed_steps(gs, slam, frames, Wm, steps, device, lambda: torch.cuda.synchronize(device))
        ms = r["step_ms"]
        q = max(len(ms) // 4, 1)
        poses = r["poses"].cpu().numpy()
        return {"frames_per_s": B * steps / r["elapsed"], "ms_per_step": r["elapsed"] / steps * 1e3,
                "ms_per_step_quartiles": [sum(ms[i * q:(i + 1) * q]) / q for i in range(4)],
                "rows_per_sequence_end": r["pc"]._tighten_counts(),
                "ate_vs_ground_truth_m": max(ate_rmse(poses[b], gt[b]) for b in range(B)), "arguments": kw}

    run()   # warm-up of every shape: allocator size classes, code objects
    run(carve_margin=MARGIN, carve_window=WINDOW)
    plain = run()
    carved = run(carve_margin=MARGIN, carve_window=WINDOW)
    plain2 = run()   # the run without carving again: the spread of the same code
    out = {"B": B, "warmup": Wm, "steps": steps, "without_carving": plain, "with_carving": carved,
           "without_carving_repeated": plain2,
           "rows_removed": [a - b for a, b in zip(plain["rows_per_sequence_end"], carved["rows_per_sequence_end"])],
           "ms_per_step_added": carved["ms_per_step"] - plain["ms_per_step"],
           "frames_per_s_ratio": carved["frames_per_s"] / plain["frames_per_s"]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("carve", "slam"), default=None)
    ap.add_argument("--steps", type=int, nargs="+", default=[20, 200])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/carve_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    if args.only in (None, "carve"):
        out["one_carve"] = carve_times(torch, gs, ops)
    if args.only in (None, "slam"):
        out["slam"] = [slam_runs(torch, gs, k, 5 if k <= 20 else 30) for k in args.steps]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
