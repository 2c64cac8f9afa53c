"""Voxel thinning: what one pass costs and what thinning does to the frame loop (needs the MI355X; fails without one).

    python tools/voxel_profile.py [--out FILE] [--only pass|slam] [--rows N [N ...]] [--steps K [K ...]]
                                  [--voxel-size V [V ...]]

1. Time of one voxel pass (gs_voxel_keep_dc_f32: the two clears of the table, elect, resolve; without the compaction that
   follows it in Pointclouds.voxel_downsample_) on one map of 2.6 M and of 10 M rows: points on a wavy sheet whose area
   grows with the row count, so that a voxel of 2^-6 m holds about 1.5 rows at either size, confidences that tie often.
     new       one ops.voxel_keep_batch call into preallocated outputs (keep and winner).
     baseline  the torch composition of the same rule (Pointclouds' path for maps the kernel does not serve, run on the
               device): floor(p / v), torch.unique over the keys with the inverse, scatter_reduce(amax) of the packed
               (score, row) words, a gather.  Both give the same integers: the outputs are compared for equality.
   Timing: device events around `reps` back-to-back calls that end in a synchronise, the two variants alternating in one
   process after a warm-up of each shape; median / min / max over the rounds.  Bytes the algorithm needs for n rows and a
   table of c slots: 2 * 16 n (point and confidence, read by both kernels) + 9 n (both outputs) + 16 c (clearing the
   table) + 16 n (one 8-byte CAS and one 8-byte max per row) + 16 n (the resolve pass's gathers of key and best, a lower
   bound: a probe sequence longer than one slot reads more).  The share of the HBM peak that these bytes over the measured
   time come to says how far a pass of scattered 8-byte atomics and gathers sits from a streaming one.

2. What thinning does to the frame loop.  The K-step B = 8 run at 640x480 (K = 200 after 30 warm-up frames; frames
   generated on the device as bench.py does), without and with PointFusion(voxel_size=V), the run without repeated for
   the spread of the same code.  Reported: frames/s, step time per quartile, final rows per sequence, ATE against
   ground truth.  Thinning adds the pass and a compaction to every step and takes rows away from every later step."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X


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


def sheet(torch, n, voxel, device, rows_per_voxel=1.5, seed=0):
    """n points on a wavy sheet of the area that gives `rows_per_voxel` rows per occupied voxel, and their confidences"""
    g = torch.Generator(device=device).manual_seed(seed)
    side = float(np.sqrt(n / rows_per_voxel) * voxel)
    xy = torch.rand((n, 2), generator=g, device=device) * side
    z = 0.3 * torch.sin(xy[:, 0]) * torch.cos(xy[:, 1]) + 0.001 * torch.randn((n,), generator=g, device=device)
    P = torch.cat([xy, z[:, None]], 1).contiguous()
    C = torch.randint(0, 8, (n, 1), generator=g, device=device).to(torch.float32) * 0.5
    return P, C


def pass_times(torch, ops, rows, voxel, reps=3, rounds=5):
    from gradslam_amd import _C
    from gradslam_amd.structures.pointclouds import _voxel_keep_torch
    device = torch.device("cuda")
    out = []
    for n in rows:
        P, C = sheet(torch, n, voxel, device)
        keep = torch.empty(n, dtype=torch.uint8, device=device)
        winner = torch.empty(n, dtype=torch.int64, device=device)
        maps = [(P, None, None, C, None, None)]
        new = lambda: ops.voxel_keep_batch(maps, voxel, out=([keep], [winner]))     # noqa: E731
        old = lambda: _voxel_keep_torch(P, C[:, 0], voxel)                           # noqa: E731
        a, o = new(), old()
        same = bool(torch.equal(a.keep[0], o[0]) and torch.equal(a.winner[0], o[1]))
        kept, unplaced = int(a.keep[0].sum()), int(a.unplaced[0])
        del a, o
        for _ in range(2):
            new(), old()
        t_new, t_old = time_pair(torch, new, old, reps, rounds)
        cap = _C.lib().gs_voxel_keep_scratch_bytes(n) // 16
        alg = 2 * 16 * n + 9 * n + 16 * cap + 16 * n + 16 * n
        s_new, s_old = stats(t_new), stats(t_old)
        rec = {"rows": n, "voxel_size": voxel, "rows_kept": kept, "unplaced": unplaced, "table_slots": cap,
               "scratch_bytes": 16 * cap, "baseline_gives_the_same_integers": same, "new": s_new, "baseline": s_old,
               "speedup_median": s_old["median_ms"] / s_new["median_ms"], "algorithmic_bytes": alg,
               "new_share_of_hbm_peak_bytes_bound": alg / (s_new["median_ms"] * 1e-3) / HBM_PEAK}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del P, C, keep, winner, maps
        torch.cuda.empty_cache()
    return out


def slam_runs(torch, gs, steps, Wm, voxels):
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
    run(voxel_size=voxels[0])
    plain = run()
    thinned = [run(voxel_size=v) for v in voxels]
    plain2 = run()   # the run without thinning again: the spread of the same code
    out = {"B": B, "warmup": Wm, "steps": steps, "without_thinning": plain, "with_thinning": thinned,
           "without_thinning_repeated": plain2,
           "frames_per_s_ratio": [t["frames_per_s"] / plain["frames_per_s"] for t in thinned]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("pass", "slam"), default=None)
    ap.add_argument("--rows", type=int, nargs="+", default=[2_600_000, 10_000_000])
    ap.add_argument("--steps", type=int, nargs="+", default=[200])
    ap.add_argument("--voxel-size", type=float, nargs="+", default=[2.0 ** -8, 2.0 ** -6])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/voxel_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    if args.only in (None, "pass"):
        out["one_pass"] = pass_times(torch, ops, args.rows, 2.0 ** -6)
    if args.only in (None, "slam"):
        out["slam"] = [slam_runs(torch, gs, k, 5 if k <= 20 else 30, args.voxel_size) for k in args.steps]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
