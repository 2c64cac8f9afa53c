"""The map prune: what one prune costs and what pruning buys the frame loop (needs the MI355X; fails without one).

    python tools/prune_profile.py [--out FILE] [--only prune|slam] [--steps K]

1. Time of one prune.  Shapes: B = 8 maps of 2.6 M surfels and B = 1 map of 10 M surfels (seeded random rows on
   buffers with room above the count, counts on the device), each with a threshold that keeps 0.5 and 0.9 of the rows.
     new       one ops.prune_map_batch call: all four attributes of all B maps, counts stay on the device.
     baseline  what the package offered before: per map a torch boolean mask on the confidence, four masked gathers
               and the count, which reads the count back (tensor[mask] has to know its size).
   The two are checked to give the same bits before anything is timed.  Timing: device events around `reps` back-to-back
   calls that end in a synchronise, the two variants alternating in one process after a warm-up of each shape; median /
   min / max over the rounds.  Bytes the algorithm needs per map of n rows with `kept` survivors (surfel layout):
   4 n (confidence, count pass) + 40 n (rows, scatter pass) + 40 kept (written); the share of the HBM peak that these
   bytes over the measured time come to is bytes-bound (the prune does no arithmetic to speak of).

2. What pruning buys.  The 200-step B = 8 run at 640x480 (30 warm-up frames, frames generated on the device as
   bench.py does for long runs), once without and once with PointFusion(prune_min_confidence=...), the threshold being
   the --quantile (default 0.5) quantile of the confidence counts the unpruned run ends with; prune_min_age and
   prune_every at their defaults.  Reported: frames/s, step time per quartile of the run, final rows per sequence, ATE
   against ground truth.  The two runs differ by design: this is a trade-off report, not a parity check."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X


def make_maps(torch, B, n, room):
    g = torch.Generator(device="cuda")
    g.manual_seed(B * 1000003 + n)
    maps = []
    for _ in range(B):
        P, N, C = (torch.randn((n + room, 3), generator=g, device="cuda") for _ in range(3))
        F = torch.rand((n + room, 1), generator=g, device="cuda")
        maps.append((P, N, C, F, n + room, torch.tensor([n], dtype=torch.int64, device="cuda")))
    return maps


def baseline(torch, maps, n, thr):
    """per map: boolean mask, four gathers, the count read back"""
    out, counts = [], []
    for P, N, C, F, _, _ in maps:
        mask = F[:n, 0] >= thr
        out.append((P[:n][mask], N[:n][mask], C[:n][mask], F[:n][mask]))
        counts.append(int(mask.sum().item()))
    return out, counts


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


def prune_times(torch, ops, reps=3, rounds=7):
    out = []
    for B, n in ((8, 2_600_000), (1, 10_000_000)):
        maps = make_maps(torch, B, n, 4096)
        for frac in (0.5, 0.9):
            thr = 1.0 - frac           # confidences are uniform in [0, 1)
            new = lambda: ops.prune_map_batch(maps, min_confidence=thr)   # noqa: E731
            old = lambda: baseline(torch, maps, n, thr)                  # noqa: E731
            r, (bo, bc) = new(), old()
            kept = r.counts.tolist()
            assert kept == bc, (kept, bc)
            for b in range(B):
                for x, y in zip(r.maps[b], bo[b]):
                    assert torch.equal(x[:kept[b]].view(torch.int32), y.view(torch.int32)), "the two variants differ"
            del r, bo
            for _ in range(2):
                new(), old()
            t_new, t_old = time_pair(torch, new, old, reps, rounds)
            alg = sum(4 * n + 40 * n + 40 * k for k in kept)
            s_new, s_old = stats(t_new), stats(t_old)
            rec = {"B": B, "rows_per_map": n, "survivor_fraction": sum(kept) / (B * n), "new": s_new, "baseline": s_old,
                   "speedup_median": s_old["median_ms"] / s_new["median_ms"], "algorithmic_bytes": alg,
                   "new_share_of_hbm_peak_bytes_bound": alg / (s_new["median_ms"] * 1e-3) / HBM_PEAK,
                   "new_no_slower": s_new["median_ms"] <= s_old["median_ms"]}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del maps
        torch.cuda.empty_cache()
    return out


def slam_runs(torch, gs, steps, quantile):
    import bench
    from gradslam_amd.metrics import ate_rmse
    B, Wm = 8, 30
    device = torch.device("cuda")
    frames, seqs = bench.make_sequences_on_device(gs, list(range(B)), Wm + steps, 480, 640, device)
    gt = np.stack([s["poses"] for s in seqs])

    def run(**kw):
        slam = gs.slam.PointFusion(odom="gradicp", device=device, **kw)
        r = bench.timed_steps(gs, slam, frames, Wm, steps, device, lambda: torch.cuda.synchronize(device))
        ms = r["step_ms"]
        q = max(len(ms) // 4, 1)
        poses = r["poses"].cpu().numpy()
        rec = {"frames_per_s": B * steps / r["elapsed"], "ms_per_step": r["elapsed"] / steps * 1e3,
               "ms_per_step_quartiles": [sum(ms[i * q:(i + 1) * q]) / q for i in range(4)],
               "rows_per_sequence_end": r["pc"]._tighten_counts(),
               "ate_vs_ground_truth_m": max(ate_rmse(poses[b], gt[b]) for b in range(B)), "arguments": kw}
        return rec, r["pc"]

    run()   # warm-up of every shape: allocator size classes, code objects
    plain, pc = run()
    cc = torch.cat([f[:, 0] for f in pc.features_list])
    thr = float(torch.quantile(cc[torch.randperm(cc.numel(), device=cc.device)[:4_000_000]].double(), quantile))
    del pc
    pruned, _ = run(prune_min_confidence=thr)
    plain2, _ = run()   # the unpruned run again: the spread of the same code
    out = {"B": B, "warmup": Wm, "steps": steps, "threshold": thr, "threshold_is": "quantile %.2f of the confidence counts the "
           "unpruned run ends with" % quantile, "without_pruning": plain, "with_pruning": pruned,
           "without_pruning_repeated": plain2,
           "ate_change_m": pruned["ate_vs_ground_truth_m"] - plain["ate_vs_ground_truth_m"],
           "frames_per_s_ratio": pruned["frames_per_s"] / plain["frames_per_s"]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("prune", "slam"), default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--quantile", type=float, default=0.5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/prune_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    if args.only in (None, "prune"):
        out["one_prune"] = prune_times(torch, ops)
    if args.only in (None, "slam"):
        out["slam_200_steps"] = slam_runs(torch, gs, args.steps, args.quantile)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
