"""The feature layers: what one fuse pass and one compaction cost, and what a layer costs the frame loop (needs the
MI355X; fails without one).

    python tools/feature_fuse_profile.py [--out FILE] [--only fuse|compact|slam] [--channels 16 64 512]

1. One fuse pass at 8 x 640 x 480 on the tables of step 10 of the bench scene (the correspondence table, depth, alpha and
   old counts that the PointFusion step hands the pass), C in --channels, float32 and float16.
     new       one ops.fuse_features_batch call for the 8 sequences.
     baseline  the torch composition of the same rule on the same tables, per sequence: index_select, arithmetic and
               index_copy_ for the matched rows, a masked gather for the appended rows (which reads a count back).
   Whether the two give the same bits is reported (the counts must agree) before anything is timed.  Timing: device
   events around `reps` back-to-back calls that end in a synchronise, the two variants alternating in one process after
   a warm-up of each shape; median / min / max over the rounds.  Algorithmic bytes per sequence: the feature image once, matched rows read
   and written (with their weights), appended rows written, and the tables (best_pix, depth, alpha, row_of_pix written
   and read: 20 B per pixel); the share of the HBM peak is these bytes over the measured time.

2. One compaction at 2.6 M rows, C = 64 and 512, float16, half of the rows kept, against boolean-mask indexing of emb
   and weight.  Algorithmic bytes: the mask twice, the kept rows read and written.

3. The 20-step PointFusion window of 8 sequences at 640 x 480 (10 warm-up frames, frames generated on the device as
   bench.py does), three times without a layer (the run-to-run spread) and twice with a C = 64 float16 layer and a
   feature image on every step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
B, H, W = 8, 480, 640


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


def tables_of_step(torch, gs, bench, step):
    """(best_pix (B, P), depth (B, H, W), alpha (B, H, W), old counts) as the pass of step `step` receives them"""
    from gradslam_amd.structures.mapfeatures import MapFeatures
    device = torch.device("cuda")
    frames, _ = bench.make_sequences_on_device(gs, list(range(B)), step + 1, H, W, device)
    slam = gs.slam.PointFusion(odom="gradicp", device=device)
    pc = gs.Pointclouds(device=device).attach_features(MapFeatures(1))
    taken, orig = [], MapFeatures._fuse

    def tap(self, pointclouds, record, depth, alpha, feat, valid):
        taken.append((record, depth, alpha))
        return orig(self, pointclouds, record, depth, alpha, feat, valid)

    MapFeatures._fuse = tap
    try:
        prev = None
        for s in range(step + 1):
            live = frames[:, s]
            pc, _ = slam.step(pc, live, prev, inplace=True)
            prev = live
    finally:
        MapFeatures._fuse = orig
    (best, n_old), depth, alpha = taken[step]
    best = best if torch.is_tensor(best) else torch.stack(list(best))
    n_old = [min(int(bound), int(n_dev.item())) if n_dev is not None else int(bound) for bound, n_dev in n_old]
    return best.clone(), depth.contiguous().clone(), alpha.contiguous().clone(), n_old


def torch_fuse(torch, emb, weight, n_old, best, depth, alpha, feat):
    """the rule as a torch composition, one sequence, in place; every pixel valid"""
    bp = best.long()
    matched = (bp >= 0) & (bp < n_old)
    pm = matched.nonzero().flatten()
    rm = bp[pm]
    a = alpha.reshape(-1)
    w, am = weight.index_select(0, rm), a[pm]
    w2 = w + am
    inv = 1.0 / torch.where(w2 == 0, torch.ones_like(w2), w2)
    e = emb.index_select(0, rm).float()
    f = feat.index_select(0, pm).float()
    emb.index_copy_(0, rm, (((w[:, None] * e) + (am[:, None] * f)) * inv[:, None]).to(emb.dtype))
    weight.index_copy_(0, rm, w2)
    new = (bp < 0) & (depth.reshape(-1) > 0)
    rows = feat[new]                      # (the masked gather: its size is read back)
    emb[n_old:n_old + rows.shape[0]] = rows
    weight[n_old:n_old + rows.shape[0]] = a[new]
    return n_old + rows.shape[0]


def fuse_times(torch, gs, ops, bench, channels, reps=3, rounds=7):
    best, depth, alpha, n_old = tables_of_step(torch, gs, bench, 10)
    P = H * W
    matched = [int(((best[b] >= 0) & (best[b] < n_old[b])).sum()) for b in range(B)]
    appended = [int(((best[b] < 0) & (depth[b].reshape(-1) > 0)).sum()) for b in range(B)]
    out = []
    for C in channels:
        for dtype in (torch.float32, torch.float16):
            es = 4 if dtype == torch.float32 else 2
            g = torch.Generator(device="cuda")
            g.manual_seed(C)
            feat = torch.randn((B, H, W, C), generator=g, device="cuda", dtype=torch.float32).to(dtype)
            mk = lambda: [(torch.randn((n_old[b] + P, C), generator=g, device="cuda", dtype=torch.float32).to(dtype),   # noqa: E731
                           torch.rand(n_old[b] + P, generator=g, device="cuda")) for b in range(B)]
            la = mk()
            lb = [(e.clone(), w.clone()) for e, w in la]
            old = [(n_old[b], None) for b in range(B)]
            new = lambda: ops.fuse_features_batch(la, old, best, depth, alpha, feat)                               # noqa: E731
            base = lambda: [torch_fuse(torch, lb[b][0], lb[b][1], n_old[b], best[b], depth[b], alpha[b],           # noqa: E731
                                       feat[b].reshape(P, C)) for b in range(B)]
            r, counts = new(), base()
            assert r.counts.tolist() == counts, (r.counts.tolist(), counts)
            view = torch.int32 if es == 4 else torch.int16
            # (reported, not asserted: the composition's arithmetic is torch's, which promises no rounding sequence)
            same = all(torch.equal(la[b][0][:counts[b]].view(view), lb[b][0][:counts[b]].view(view)) and
                       torch.equal(la[b][1][:counts[b]].view(torch.int32), lb[b][1][:counts[b]].view(torch.int32))
                       for b in range(B))
            for _ in range(2):
                new(), base()
            t_new, t_old = time_pair(torch, new, base, reps, rounds)
            row = C * es
            alg = sum(P * row + 2 * matched[b] * (row + 4) + appended[b] * (row + 4) + 20 * P for b in range(B))
            s_new, s_old = stats(t_new), stats(t_old)
            rec = {"B": B, "H": H, "W": W, "C": C, "dtype": str(dtype).split(".")[-1], "rows_before": n_old,
                   "matched_pixels": matched, "appended_pixels": appended, "same_bits_as_baseline": same,
                   "new": s_new, "baseline": s_old,
                   "speedup_median": s_old["median_ms"] / s_new["median_ms"], "algorithmic_bytes": alg,
                   "new_bytes_per_s": alg / (s_new["median_ms"] * 1e-3),
                   "new_share_of_hbm_peak": alg / (s_new["median_ms"] * 1e-3) / HBM_PEAK}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del la, lb, feat
            torch.cuda.empty_cache()
    return out


def compact_times(torch, ops, reps=3, rounds=7):
    out, n = [], 2_600_000
    for C in (64, 512):
        g = torch.Generator(device="cuda")
        g.manual_seed(C)
        emb = torch.randn((n, C), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        weight = torch.rand(n, generator=g, device="cuda")
        keep = (torch.rand(n, generator=g, device="cuda") < 0.5)
        keep8 = keep.to(torch.uint8)
        dst = [(torch.empty_like(emb), torch.empty_like(weight))]
        new = lambda: ops.compact_features_batch([(emb, weight)], [(n, None)], [keep8], out=dst)     # noqa: E731
        base = lambda: (emb[keep], weight[keep])                                                        # noqa: E731
        r, (be, bw) = new(), base()
        kept = int(r.counts[0])
        assert kept == be.shape[0] and torch.equal(dst[0][0][:kept].view(torch.int16), be.view(torch.int16))
        assert torch.equal(dst[0][1][:kept].view(torch.int32), bw.view(torch.int32))
        del be, bw
        for _ in range(2):
            new(), base()
        t_new, t_old = time_pair(torch, new, base, reps, rounds)
        alg = 2 * n + 2 * kept * (2 * C + 4)
        s_new, s_old = stats(t_new), stats(t_old)
        rec = {"rows": n, "C": C, "dtype": "float16", "kept": kept, "new": s_new, "baseline": s_old,
               "speedup_median": s_old["median_ms"] / s_new["median_ms"], "algorithmic_bytes": alg,
               "new_bytes_per_s": alg / (s_new["median_ms"] * 1e-3),
               "new_share_of_hbm_peak": alg / (s_new["median_ms"] * 1e-3) / HBM_PEAK}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del emb, weight, dst
        torch.cuda.empty_cache()
    return out


def slam_window(torch, gs, bench, warmup=10, steps=20, C=64):
    from gradslam_amd.structures.mapfeatures import MapFeatures
    device = torch.device("cuda")
    frames, _ = bench.make_sequences_on_device(gs, list(range(B)), warmup + steps, H, W, device)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    feat = torch.randn((B, H, W, C), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)

    def run(layer):
        slam = gs.slam.PointFusion(odom="gradicp", device=device)
        pc = gs.Pointclouds(device=device)
        if layer:
            pc.attach_features(MapFeatures(C, torch.float16))
        more = dict(features=feat) if layer else {}
        prev = None
        for s in range(warmup + steps):
            if s == warmup:
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
            live = frames[:, s]
            pc, _ = slam.step(pc, live, prev, inplace=True, **more)
            prev = live
        torch.cuda.synchronize(device)
        el = time.perf_counter() - t0
        return {"frames_per_s": B * steps / el, "ms_per_step": el / steps * 1e3}

    run(False), run(True)     # warm-up of every shape: allocator size classes, code objects
    out = {"B": B, "H": H, "W": W, "warmup": warmup, "steps": steps, "C": C, "dtype": "float16",
           "without_layer": [run(False) for _ in range(3)], "with_layer": [run(True) for _ in range(2)]}
    out["with_over_without_frames_per_s"] = (statistics.median(r["frames_per_s"] for r in out["with_layer"]) /
                                             statistics.median(r["frames_per_s"] for r in out["without_layer"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fuse", "compact", "slam"), default=None)
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 512])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/feature_fuse_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import bench
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    if args.only in (None, "fuse"):
        out["one_fuse_pass"] = fuse_times(torch, gs, ops, bench, args.channels)
    if args.only in (None, "compact"):
        out["one_compaction"] = compact_times(torch, ops)
    if args.only in (None, "slam"):
        out["slam_window"] = slam_window(torch, gs, bench)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
