"""The bilateral depth filter: what one launch costs and what the pre-pass costs the frame loop (needs the MI355X; fails
without one).

    python tools/bilateral_profile.py [--out FILE] [--only launch|slam] [--steps K]

1. Time of one launch.  B = 8 frames of 640x480 (the synthetic surface with 4 mm of noise and 5 % holes), radius 1, 3
   and 8, sigma_space 2 px, sigma_range 0.03 m.
     new       one ops.bilateral_depth call (gs_bilateral_depth_f32), and the call with its backward.
     baseline  the composition a user would write in torch: F.unfold of the padded stack ((2r+1)^2 copies of every
               frame), exp of the two squared distances, masked sums, a division.
   The two are checked to agree to 1e-5 m before anything is timed (torch's exp is not the pinned one, so not in
   bits).  Timing: device events around `reps` back-to-back calls that end in a synchronise, the two variants alternating
   in one process after a warm-up of each shape; median / min / max over the rounds.  Reported next to the time: the
   share of the HBM peak that the 8 B per pixel the algorithm needs come to, and exps per second ((2r+1)^2 per valid
   pixel) -- the kernel is expected to be bound by the exp chain out of LDS, not by bytes.

2. What the pre-pass costs.  A 20-step window of the B = 8 run at 640x480 (10 warm-up frames) with PointFusion() and
   with PointFusion(depth_filter=dict(radius=3, ...)): frames/s and ms per step of both, and the unfiltered run
   repeated for the spread of the same code.  The results differ by design; this is a cost report, not a parity check."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
SIGMA_SPACE, SIGMA_RANGE = 2.0, 0.03


def noisy_stack(torch, B, H, W):
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(1, H, W, seed=0)
    d = torch.from_numpy(s["depths"][0, ..., 0]).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    stack = d.unsqueeze(0).repeat(B, 1, 1)
    noise = 0.004 * torch.randn(stack.shape, generator=g, device="cuda")
    return torch.where(stack > 0, stack + noise, stack).contiguous()


def unfold_baseline(torch, depth, radius):
    """the torch composition: (n, H, W) -> (n, H, W)"""
    import torch.nn.functional as F
    n, H, W = depth.shape
    k = 2 * radius + 1
    valid = depth > 0
    dz = torch.where(valid, depth, torch.zeros_like(depth))
    cols = F.unfold(dz.unsqueeze(1), k, padding=radius).view(n, k * k, H, W)
    ax = torch.arange(-radius, radius + 1, device=depth.device, dtype=depth.dtype)
    g = torch.exp(-(ax.view(-1, 1) ** 2 + ax.view(1, -1) ** 2) / (2 * SIGMA_SPACE ** 2)).view(1, k * k, 1, 1)
    w = g * torch.exp(-(cols - dz.unsqueeze(1)) ** 2 / (2 * SIGMA_RANGE ** 2)) * (cols > 0)
    out = (w * cols).sum(1) / w.sum(1).clamp_min(1e-30)
    return torch.where(valid, out, depth)


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


def launch_times(torch, ops, reps=5, rounds=7):
    B, H, W = 8, 480, 640
    depth = noisy_stack(torch, B, H, W)
    n_valid = int((depth > 0).sum())
    out = []
    for radius in (1, 3, 8):
        kw = dict(radius=radius, sigma_space=SIGMA_SPACE, sigma_range=SIGMA_RANGE)
        buf = torch.empty_like(depth)
        new = lambda: ops.bilateral_depth(depth, out=buf, **kw)          # noqa: E731
        old = lambda: unfold_baseline(torch, depth, radius)             # noqa: E731
        diff = float((new() - old()).abs().max())
        assert diff < 1e-5, "the two variants differ by %g m" % diff
        leaf = depth.clone().requires_grad_(True)
        ob = torch.ones_like(depth)

        def both():
            leaf.grad = None
            ops.bilateral_depth(leaf, **kw).backward(ob)

        for _ in range(2):
            new(), old(), both()
        t_new, t_old = time_pair(torch, new, old, reps, rounds)
        t_both, _ = time_pair(torch, both, new, reps, rounds)
        s_new, s_old, s_both = stats(t_new), stats(t_old), stats(t_both)
        sec = s_new["median_ms"] * 1e-3
        rec = {"B": B, "H": H, "W": W, "radius": radius, "max_abs_difference_m": diff, "new": s_new, "baseline_unfold": s_old,
               "new_forward_plus_backward": s_both, "speedup_median": s_old["median_ms"] / s_new["median_ms"],
               "algorithmic_bytes": 8 * B * H * W, "share_of_hbm_peak": 8 * B * H * W / sec / HBM_PEAK,
               "exps_per_s": n_valid * (2 * radius + 1) ** 2 / sec}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def slam_runs(torch, gs, steps, warmup=10):
    import bench
    B = 8
    device = torch.device("cuda")
    frames, _ = bench.make_sequences_on_device(gs, list(range(B)), warmup + steps, 480, 640, device)

    def run(**kw):
        slam = gs.slam.PointFusion(odom="gradicp", device=device, **kw)
        r = bench.timed_steps(gs, slam, frames, warmup, steps, device, lambda: torch.cuda.synchronize(device))
        return {"frames_per_s": B * steps / r["elapsed"], "ms_per_step": r["elapsed"] / steps * 1e3,
                "gpu_ms_per_step_median": statistics.median(r["step_ms"]), "arguments": {k: dict(v) for k, v in kw.items()}}

    flt = dict(radius=3, sigma_space=SIGMA_SPACE, sigma_range=SIGMA_RANGE)
    run(), run(depth_filter=flt)   # warm-up of every shape: allocator size classes, code objects
    plain = run()
    filtered = run(depth_filter=flt)
    plain2 = run()
    out = {"B": B, "warmup": warmup, "steps": steps, "without_filter": plain, "with_filter": filtered,
           "without_filter_repeated": plain2, "frames_per_s_ratio": filtered["frames_per_s"] / plain["frames_per_s"]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("launch", "slam"), default=None)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bilateral_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    if args.only in (None, "launch"):
        out["one_launch"] = launch_times(torch, ops)
    if args.only in (None, "slam"):
        out["slam_window"] = slam_runs(torch, gs, args.steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
