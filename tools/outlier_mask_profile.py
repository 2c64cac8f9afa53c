"""The projective ICP's outlier mask: what the mask costs and what the frame loop pays for it (needs the MI355X; fails
without one).

    python tools/outlier_mask_profile.py [--out FILE] [--only mask|slam] [--steps K]

1. The mask.  640x480 frames of the benchmark's synthetic sequences, the map fused from the first 10 frames under the
   ground-truth poses, frame 10 at the pose of frame 9 against the model view rendered there; B = 1 and B = 8.
     mask_grow0 / mask_grow8 / mask_grow16   ops.projective_icp_outliers_batch: the residual pass, the median's select,
                       the class pass and the region pass (the counters' clear in front), grow = 0, 8, 16
     region_grow0 / region_grow8 / region_grow16   ops.region_mask alone on the class image of that call
     iteration_stride1 one iteration of ops.projective_icp_batch(huber_k=1.345) at stride 1: the yardstick the mask was
                       expected to cost about as much as (four launches over the same pixels)
   Timing: device events around `reps` back-to-back calls that end in a synchronise, the variants alternating in one
   process after a warm-up of each; median / min / max over the rounds.

2. The frame loop.  A 20-step window of the B = 8 run at 640x480 (10 warm-up frames) of PointFusion(odom="projicp",
   huber_k=1.345) without the mask, with odom_outlier_mask={} (the defaults: 5 more iterations) and with
   fuse_outliers=False on top, the plain run repeated for the spread of the same code: frames/s, ms per step and the ATE
   (RMSE of the translation error against the ground truth over the timed frames)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import projective_icp_profile as pip   # noqa: E402  (the scene, the round-robin timer and the window of the sibling tool)

K_HUBER = 1.345
GROWS = (0, 8, 16)


def mask_times(torch, gs, ops, reps=5, rounds=7):
    out = []
    for B in (1, 8):
        pc, live, prev, _ = pip.scene(torch, gs, B)
        fr = live.to_channels_last()
        K = fr.intrinsics[:, 0].contiguous()
        H, W = fr.shape[2:4]
        maps = pc._map_rows(("points", "normals"))
        p0 = prev[:, 0].contiguous()
        index = ops.render_map_batch([m._replace(normals=None) for m in maps], prev, K, H, W).index[:, 0]
        args = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, index, p0, maps, p0)
        classes = ops.projective_icp_outliers_batch(*args, return_classes=True)[1]
        depth = args[2].contiguous()
        fns = {"iteration_stride1": lambda: ops.projective_icp_batch(*args, stride=1, numiters=1, huber_k=K_HUBER)}
        for g in GROWS:
            fns["mask_grow%d" % g] = lambda g=g: ops.projective_icp_outliers_batch(*args, grow=g)
            fns["region_grow%d" % g] = lambda g=g: ops.region_mask(classes, depth, grow=g)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        res = {"B": B, "H": int(H), "W": int(W), "masked_fraction": float(fns["mask_grow0"]().float().mean())}
        res.update(pip.time_round_robin(torch, fns, reps, rounds))
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


def slam_runs(torch, gs, steps, warmup=10):
    import statistics

    import bench
    B = 8
    device = torch.device("cuda")
    frames, gt = bench.make_sequences_on_device(gs, list(range(B)), warmup + steps, pip.H, pip.W, device)
    gt_t = torch.from_numpy(gt[0]["poses"][warmup:warmup + steps, :3, 3]).to(device).double()

    def run(**kw):
        slam = gs.slam.PointFusion(odom="projicp", device=device, huber_k=K_HUBER, **kw)
        r = bench.timed_steps(gs, slam, frames, warmup, steps, device, lambda: torch.cuda.synchronize(device))
        e = (r["poses"][:, warmup:warmup + steps, :3, 3].double() - gt_t).norm(dim=-1)
        return {"frames_per_s": B * steps / r["elapsed"], "ms_per_step": r["elapsed"] / steps * 1e3,
                "gpu_ms_per_step_median": statistics.median(r["step_ms"]), "ate_rmse_m": float((e * e).mean().sqrt())}

    variants = {"plain": dict(), "masked": dict(odom_outlier_mask={}),
                "masked_not_fused": dict(odom_outlier_mask={}, fuse_outliers=False)}
    for kw in variants.values():   # warm-up of every shape: allocator size classes, code objects
        run(**kw)
    out = {"B": B, "H": pip.H, "W": pip.W, "warmup": warmup, "steps": steps, "huber_k": K_HUBER}
    for name, kw in variants.items():
        out[name] = run(**kw)
    out["plain_repeated"] = run()
    out["ms_per_step_extra_masked"] = out["masked"]["ms_per_step"] - out["plain"]["ms_per_step"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("mask", "slam"), default=None)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/outlier_mask_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0)}
    if args.only in (None, "mask"):
        out["mask"] = mask_times(torch, gs, ops)
    if args.only in (None, "slam"):
        out["slam_window"] = slam_runs(torch, gs, args.steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
