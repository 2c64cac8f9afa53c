"""The model view against the composition the package offered before it (needs the MI355X).

    python tools/render_profile.py [--out FILE]                 timed comparison, both sizes
    python tools/render_profile.py --trace-run small|large      only the new call, N times (run it under
                                                                rocprofv3 --kernel-trace --stats, no counters)
    python tools/render_profile.py --kernel-stats small=CSV large=CSV [--out FILE]
                                                                algorithmic bytes over the kernel times of those runs
    python tools/render_profile.py --backward [--out FILE]      forward and backward of the differentiable render, timed
    python tools/render_profile.py --projicp-window [--json FILE]  (also in a checkout of the parent commit: its side)
    python tools/render_profile.py --radii [--steps 20 200] [--json FILE] [--parent-json FILE] [--out FILE]
                                                                the view with per-surfel radii against radius 0, 1 and 3,
                                                                and a projective-ICP window with and without them

new       one Pointclouds.render call, one view, all five images.
baseline  the same five images from ops.project_map + ops.transform_points + int64 key packing +
          Tensor.scatter_reduce_("amin") + gathers; checked to give the same bits as the new call before anything is
          timed.

Sizes: `small` = the 640x480 map of one sequence of the benchmark after its 5 + 20 frames (PointFusion, gradICP
odometry, seed 0; about 0.9 M surfels), seen from the last pose; `large` = a 1296x968 view of 10 M surfels laid out in
the view's frustum by a seeded generator (a PointFusion run of that size takes minutes of host-side frame synthesis):
rows land on uniformly random pixels, about 8 per pixel, their depths within +-1 cm of a smooth surface 1.5 - 2.5 m
away, so that, as in a fused map, the rows of a pixel compete at nearly equal depth.

Timing: device events around `reps` back-to-back calls (a window well above a millisecond), the two variants
alternating in one process, after a warm-up of each shape; median / min / max over the rounds."""
import argparse
import csv
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X


def camera_inverse(pose):
    """float32 [R^T | ti] and [R^T | 0] of a camera-to-world pose, ti in the kernels' arithmetic (gs_camera: plain
    left-to-right dot of the negated rows with t)."""
    pose = np.asarray(pose, np.float32).reshape(4, 4)
    Rt = np.ascontiguousarray(pose[:3, :3].T)
    t = pose[:3, 3]
    Tinv = np.eye(4, dtype=np.float32)
    Tinv[:3, :3] = Rt
    for j in range(3):
        Tinv[j, 3] = np.float32(np.float32(np.float32(-Rt[j, 0]) * t[0] + np.float32(-Rt[j, 1]) * t[1]) + np.float32(-Rt[j, 2]) * t[2])
    Trot = Tinv.copy()
    Trot[:3, 3] = 0
    return Tinv, Trot


def small_case(gs, torch):
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(25, 480, 640, seed=0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    poses = T(s["poses"][None])
    poses[:, 1:] = poses[:, :1]
    frames = gs.RGBDImages(T(s["colors"][None]), T(s["depths"][None]), T(s["intrinsics"][None]), poses)
    pc, rec = gs.slam.PointFusion(odom="gradicp", device="cuda")(frames)
    return pc, frames.intrinsics, rec[:, -1:].contiguous(), 480, 640


def large_case(gs, torch, n=10_000_000, H=968, W=1296):
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    fx = fy = 1.2 * W / 2
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u = torch.rand(n, generator=g, device="cuda") * (W - 1)
    v = torch.rand(n, generator=g, device="cuda") * (H - 1)
    z = 2.0 + 0.5 * torch.sin(u * (3.0 / W)) * torch.cos(v * (2.0 / H)) + (torch.rand(n, generator=g, device="cuda") - 0.5) * 0.02
    P = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1).contiguous()
    N = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, device="cuda") * 0.2 + torch.tensor([0.0, 0.0, 1.0], device="cuda"), dim=-1)
    C = torch.rand(n, 3, generator=g, device="cuda") * 255
    F = torch.rand(n, 1, generator=g, device="cuda") * 10 + 0.01
    K = torch.tensor([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device="cuda")
    pc = gs.Pointclouds(points=[P], normals=[N.contiguous()], colors=[C], features=[F])
    return pc, K.reshape(1, 1, 4, 4), torch.eye(4, device="cuda").reshape(1, 1, 4, 4), H, W


def make_baseline(torch, ops, pc, K, pose, H, W):
    """the five images of one view from the calls the package had before the renderer"""
    P, N, C, F = (pc._buf[k][0] for k in ("points", "normals", "colors", "features"))
    n = int(pc.num_points_per_pointcloud[0])
    P, N, C, F = P[:n], N[:n], C[:n], F[:n]
    Tinv, Trot = (torch.from_numpy(a).cuda() for a in camera_inverse(pose[0, 0].cpu().numpy()))
    K4, T4 = K[0, 0].contiguous(), pose[0, 0].contiguous()
    EMPTY = torch.iinfo(torch.int64).max
    mode = {"how": "scatter_reduce_(amin) on int64 keys"}

    def run():
        pix = ops.project_map(P, T4, K4, H, W)
        q = ops.transform_points(P, Tinv)
        key = (q[:, 2].contiguous().view(torch.int32).to(torch.int64) << 32) | torch.arange(n, device="cuda")
        sel = pix >= 0
        keys = torch.full((H * W,), EMPTY, dtype=torch.int64, device="cuda")
        if mode["how"].startswith("scatter"):
            keys.scatter_reduce_(0, pix[sel].to(torch.int64), key[sel], "amin")
        else:   # two stable sorts: by key, then by pixel; the first row of every pixel group wins
            ks, ps = key[sel], pix[sel].to(torch.int64)
            o1 = torch.sort(ks, stable=True).indices
            o2 = torch.sort(ps[o1], stable=True)
            ks, ps = ks[o1][o2.indices], o2.values
            first = torch.ones_like(ps, dtype=torch.bool)
            first[1:] = ps[1:] != ps[:-1]
            keys[ps[first]] = ks[first]
        hit = keys != EMPTY
        row = torch.where(hit, keys & 0xFFFFFFFF, torch.zeros_like(keys))
        zero = torch.zeros((), device="cuda")
        depth = torch.where(hit, (keys >> 32).to(torch.int32).view(torch.float32), zero)
        nc = ops.transform_points(N, Trot)
        h3 = hit.unsqueeze(-1)
        return (depth.view(H, W, 1), torch.where(h3, C[row], zero).view(H, W, 3), torch.where(h3, nc[row], zero).view(H, W, 3),
                torch.where(hit, F[row, 0], zero).view(H, W, 1), torch.where(hit, row, torch.full_like(row, -1)).view(H, W))

    try:
        run()
        torch.cuda.synchronize()
    except (RuntimeError, NotImplementedError) as e:
        mode["how"] = "two stable sorts (scatter_reduce_ amin on int64 failed: %s)" % str(e).splitlines()[0][:80]
        run()
    return run, mode, n


def algorithmic_bytes(n, H, W, hits):
    """key pass 12 B per row; resolve 8 B key read + 40 B of images per pixel + 28 B gathered per
    covered pixel (colour 12, normal 12, count 4); the clear writes 8 B per pixel."""
    return {"key": 12.0 * n, "resolve": 48.0 * H * W + 28.0 * hits, "clear": 8.0 * H * W}


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # microseconds per call


def compare(out):
    import torch
    import gradslam_amd as gs
    from gradslam_amd import ops
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = ["# tools/render_profile.py: Pointclouds.render (one view, five images) against project_map + transform_points +",
             "# int64 keys + scatter_reduce_(amin) + gathers; microseconds per call, device events, variants alternating"]
    ok = True
    for name, case in (("small", small_case), ("large", large_case)):
        pc, K, pose, H, W = case(gs, torch)
        base, mode, n = make_baseline(torch, ops, pc, K, pose, H, W)

        def new():
            return pc.render(K, pose, H, W, return_extras=True)
        r, ex = new()
        got = (r.depth_image[0, 0], r.rgb_image[0, 0], ex["normal"][0, 0], ex["confidence"][0, 0], ex["index"][0, 0])
        want = base()
        for k, a, b in zip(("depth", "color", "normal", "confidence", "index"), got, want):
            assert a.shape == b.shape and torch.equal(a, b), "%s: the baseline and the new call differ in %s" % (name, k)
        hits = int((got[4] >= 0).sum())
        for _ in range(3):
            new(), base()
        torch.cuda.synchronize()
        t_new = timed(torch, new, 20)
        t_base = timed(torch, base, 5)
        reps_new, reps_base = max(10, int(math.ceil(5000.0 / t_new))), max(3, int(math.ceil(5000.0 / t_base)))
        rn, rb = [], []
        for _ in range(9):
            rn.append(timed(torch, new, reps_new))
            rb.append(timed(torch, base, reps_base))
        med = lambda x: float(np.median(x))  # noqa: E731
        ratio = med(rb) / med(rn)
        ok = ok and max(rn) < min(rb)
        by = algorithmic_bytes(n, H, W, hits)
        lines += ["", "## %s: %d x %d view of %d surfels, %d of %d pixels covered; same bits as the baseline: yes" % (name, W, H, n, hits, H * W),
                  "baseline composition: %s" % mode["how"],
                  "new       median %9.1f us   min %9.1f   max %9.1f   (%d calls per window, 9 windows)" % (med(rn), min(rn), max(rn), reps_new),
                  "baseline  median %9.1f us   min %9.1f   max %9.1f   (%d calls per window, 9 windows)" % (med(rb), min(rb), max(rb), reps_base),
                  "baseline / new = %.1f   (worst new window against best baseline window: %.1f)" % (ratio, min(rb) / max(rn)),
                  "algorithmic bytes per call: key pass %.1f MB, resolve %.1f MB, clear %.1f MB; all of them over the call time: %.2f TB/s"
                  % (by["key"] / 1e6, by["resolve"] / 1e6, by["clear"] / 1e6, sum(by.values()) / (med(rn) * 1e-6) / 1e12)]
        del pc, base
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)
    if not ok:
        sys.exit("the new call is not ahead of the baseline at both sizes")


def two_frame_case(gs, torch):
    """the 480x640 map of two frames (ground-truth odometry) seen from its second pose"""
    from gradslam_amd.datasets.synthetic import make_sequence
    s = make_sequence(2, 480, 640, seed=5)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    frames = gs.RGBDImages(T(s["colors"][None]), T(s["depths"][None]), T(s["intrinsics"][None]), T(s["poses"][None]))
    pc, _ = gs.slam.PointFusion(odom="gt", device="cuda")(frames)
    return pc, frames.intrinsics, frames.poses[:, 1:].contiguous(), 480, 640


def backward_times(out):
    """Forward (the plain render, five images) and backward (gs_render_map_backward_dc_f32 through autograd: all four
    upstream images, gradients for the four map attributes and the pose) of one view, microseconds per call."""
    import torch
    import gradslam_amd as gs
    from gradslam_amd import ops
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = ["# tools/render_profile.py --backward: ops.render_map (one view, five images) and the backward of",
             "# ops.render_map(differentiable=True) (torch.autograd.grad: four upstream images -> points, normals, colours, counts,",
             "# pose); microseconds per call, device events, forward and backward windows alternating"]
    for name, case, radius in (("two-frame 640x480", two_frame_case, 0), ("two-frame 640x480", two_frame_case, 1),
                               ("large", large_case, 0)):
        pc, K, pose, H, W = case(gs, torch)
        n = int(pc.num_points_per_pointcloud[0])
        leaves = [pc._buf[k][0][:n].detach().clone().requires_grad_(True) for k in ("points", "normals", "colors", "features")]
        T4 = pose[0].detach().clone().requires_grad_(True)
        K4 = K[0, 0].contiguous()
        plain = [t.detach() for t in leaves]

        def fwd():
            return ops.render_map(*plain, T4.detach(), K4, H, W, radius=radius)
        r = ops.render_map(*leaves, T4, K4, H, W, radius=radius, differentiable=True)
        outs = [r.depth, r.color, r.normal, r.confidence]
        ups = [torch.randn_like(t) for t in outs]

        def bwd():
            return torch.autograd.grad(outs, leaves + [T4], ups, retain_graph=True)
        hits = int((r.index >= 0).sum())
        for _ in range(3):
            fwd(), bwd()
        torch.cuda.synchronize()
        reps_f = max(10, int(math.ceil(5000.0 / timed(torch, fwd, 10))))
        reps_b = max(10, int(math.ceil(5000.0 / timed(torch, bwd, 10))))
        tf, tb = [], []
        for _ in range(9):
            tf.append(timed(torch, fwd, reps_f))
            tb.append(timed(torch, bwd, reps_b))
        med = lambda x: float(np.median(x))  # noqa: E731
        lines += ["", "## %s, radius %d: %d x %d view of %d surfels, %d of %d pixels covered" % (name, radius, W, H, n, hits, H * W),
                  "forward   median %9.1f us   min %9.1f   max %9.1f   (%d calls per window, 9 windows)" % (med(tf), min(tf), max(tf), reps_f),
                  "backward  median %9.1f us   min %9.1f   max %9.1f   (%d calls per window, 9 windows)" % (med(tb), min(tb), max(tb), reps_b),
                  "backward / forward = %.2f" % (med(tb) / med(tf))]
        del pc, leaves, plain, r, outs, ups
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def projicp_window(layer_kw=None, runs=3):
    """ms per step of 20 steps of PointFusion(odom="projicp") on one 640x480 sequence of the benchmark scene after 5
    frames, `runs` times (wall time, device idle at both ends).  layer_kw None: no layer, calls that every version of the
    package with odom="projicp" has -- `python tools/render_profile.py --projicp-window --json FILE` in a checkout of the
    parent commit (with this file copied in) gives the other side of the comparison; else the map carries a SurfelRadii
    layer and the driver takes layer_kw."""
    import time
    import torch
    import gradslam_amd as gs
    from gradslam_amd.datasets.synthetic import make_sequence
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    s = make_sequence(25, 480, 640, seed=0)
    out = []
    for _ in range(runs):
        poses = T(s["poses"][None])
        poses[:, 1:] = poses[:, :1]
        frames = gs.RGBDImages(T(s["colors"][None]), T(s["depths"][None]), T(s["intrinsics"][None]), poses)
        if layer_kw is None:
            slam, pc = gs.slam.PointFusion(odom="projicp", device="cuda"), gs.Pointclouds(device="cuda")
        else:
            slam = gs.slam.PointFusion(odom="projicp", device="cuda", surfel_radii=True, **layer_kw)
            pc = gs.Pointclouds(device="cuda").attach_features(gs.SurfelRadii())
        prev = None
        for f in range(25):
            if f == 5:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            live = frames[:, f]
            pc, _ = slam.step(pc, live, prev, inplace=True)
            prev = live
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / 20 * 1e3)
    return out


def radii_times(steps, out, json_out, parent_json=None):
    """The model view with the radii of a SurfelRadii layer (Pointclouds.render(radii="layer"), max_radius 3) against the
    constant radii 0, 1 and 3: one 640x480 view, index and depth image only (what the projective ICP renders: the key
    pass dominates), of the map of one sequence of the benchmark scene after `steps` frames (PointFusion, gradICP
    odometry, seed 0), seen from the last pose -- from where the map was built.  Then a window of 20 steps of
    PointFusion(odom="projicp") on a map of 5 frames (projicp_window): without a layer, with the layer, and with the layer
    and odom_surfel_radii, three runs each; parent_json: the figures of --projicp-window from a checkout of the parent
    commit, which go into the report next to them."""
    import json
    import torch
    import gradslam_amd as gs
    from gradslam_amd import ops
    from gradslam_amd.datasets.synthetic import make_sequence
    assert torch.cuda.is_available(), "needs the MI355X"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    H, W = 480, 640
    report = {"tool": "tools/render_profile.py --radii", "size": [H, W], "views": []}
    lines = ["# tools/render_profile.py --radii: ops.render_map_batch (one 640x480 view, depth and index) with radius 0 / 1 / 3",
             "# and with the radii of the map's SurfelRadii layer (max_radius 3); microseconds per call, device events, the",
             "# variants alternating"]
    med = lambda x: float(np.median(x))  # noqa: E731
    for n_steps in steps:
        s = make_sequence(n_steps, H, W, seed=0)
        poses = T(s["poses"][None])
        poses[:, 1:] = poses[:, :1]
        frames = gs.RGBDImages(T(s["colors"][None]), T(s["depths"][None]), T(s["intrinsics"][None]), poses)
        pc, rec = gs.slam.PointFusion(odom="gradicp", device="cuda", surfel_radii=True)(frames)
        n = int(pc.num_points_per_pointcloud[0])
        maps = [m._replace(normals=None, colors=None, features=None) for m in pc._map_rows()]
        radii = [t.contiguous() for t in pc.map_features.radii_list]
        K, pose = frames.intrinsics[:, 0].contiguous(), rec[:, -1:].contiguous()
        calls = {"radius=%d" % r: (lambda r=r: ops.render_map_batch(maps, pose, K, H, W, radius=r)) for r in (0, 1, 3)}
        calls["radii"] = lambda: ops.render_map_batch(maps, pose, K, H, W, radii=radii, max_radius=3)
        calls["radii, cap 8"] = lambda: ops.render_map_batch(maps, pose, K, H, W, radii=radii, max_radius=8)
        # the same map from half the distance along the optical axis of the last pose: wider squares
        near = pose.clone()
        near[:, 0, :3, 3] += 1.0 * pose[:, 0, :3, 2]
        calls["radius=1, 1 m nearer"] = lambda: ops.render_map_batch(maps, near, K, H, W, radius=1)
        calls["radii, 1 m nearer"] = lambda: ops.render_map_batch(maps, near, K, H, W, radii=radii, max_radius=3)
        calls["radii, cap 8, 1 m nearer"] = lambda: ops.render_map_batch(maps, near, K, H, W, radii=radii, max_radius=8)
        view = {"steps": n_steps, "surfels": n, "us": {}, "covered": {}}
        for k, fn in calls.items():
            for _ in range(3):
                fn()
            view["covered"][k] = int((fn().index >= 0).sum())
        torch.cuda.synchronize()
        reps = {k: max(10, int(math.ceil(5000.0 / timed(torch, fn, 10)))) for k, fn in calls.items()}
        t = {k: [] for k in calls}
        for _ in range(9):
            for k, fn in calls.items():
                t[k].append(timed(torch, fn, reps[k]))
        fb = float(K[0, 0, 0] + K[0, 1, 1]) / 2
        lines += ["", "## after %d steps: %d surfels, mean radius %.2f mm (%.2f px at 2 m)"
                  % (n_steps, n, 1e3 * float(radii[0].mean()), float(radii[0].mean()) * fb / 2.0)]
        for k in calls:
            view["us"][k] = {"median": med(t[k]), "min": min(t[k]), "max": max(t[k])}
            lines.append("%-26s median %9.1f us   min %9.1f   max %9.1f   covered %d of %d"
                         % (k, med(t[k]), min(t[k]), max(t[k]), view["covered"][k], H * W))
        report["views"].append(view)
        del pc, frames, maps, radii
        torch.cuda.empty_cache()
    # the tracking window
    window = {"steps": 20, "ms_per_step": {}}
    for name, kw in (("projicp", None), ("projicp, SurfelRadii layer", {}),
                     ("projicp, SurfelRadii layer, odom_surfel_radii", dict(odom_surfel_radii=True))):
        runs = projicp_window(kw)
        window["ms_per_step"][name] = runs
        lines.append("%-46s 20 steps after 5: %s ms per step (three runs)" % (name, ", ".join("%.3f" % x for x in runs)))
    if parent_json:
        window["ms_per_step"]["projicp, parent commit"] = runs = json.load(open(parent_json))["ms_per_step"]
        lines.append("%-46s 20 steps after 5: %s ms per step (three runs)" % ("projicp, parent commit",
                                                                              ", ".join("%.3f" % x for x in runs)))
    report["projicp_window"] = window
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)
    if json_out:
        with open(json_out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")


def trace_run(which, calls=30):
    import torch
    import gradslam_amd as gs
    pc, K, pose, H, W = (small_case if which == "small" else large_case)(gs, torch)
    for _ in range(calls):
        r, ex = pc.render(K, pose, H, W, return_extras=True)
    torch.cuda.synchronize()
    print("RENDER_TRACE %s n=%d H=%d W=%d hits=%d" % (which, int(pc.num_points_per_pointcloud[0]), H, W, int((ex["index"] >= 0).sum())))


def kernel_stats(pairs, out):
    lines = ["", "# kernel times (rocprofv3 --kernel-trace --stats, a run of its own per size, 30 calls each) and the algorithmic",
             "# bytes of DESIGN.md section 4 over them; share of the 8.0 TB/s HBM3E specification"]
    for p in pairs:
        name, path, n, H, W, hits = p.split("=")[0], p.split("=")[1].split(",")[0], *[int(x) for x in p.split("=")[1].split(",")[1:]]
        by = algorithmic_bytes(n, H, W, hits)
        lines.append("## %s: n=%d, %dx%d, %d covered pixels" % (name, n, W, H, hits))
        for r in csv.DictReader(open(path)):
            if "gs_render_" not in r["Name"]:
                continue
            kind = "key" if "key_kernel" in r["Name"] else "resolve"
            avg = float(r["AverageNs"])
            rate = by[kind] / (avg * 1e-9)
            lines.append("%-26s calls %4s  avg %9.2f us  min %9.2f  max %9.2f   %7.1f MB -> %5.2f TB/s = %4.1f %% of HBM peak" % (
                "gs_render_%s_kernel" % kind, r["Calls"], avg / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, by[kind] / 1e6,
                rate / 1e12, 100.0 * rate / HBM_PEAK))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the report to this file")
    ap.add_argument("--trace-run", choices=["small", "large"], default=None)
    ap.add_argument("--kernel-stats", nargs="+", metavar="NAME=CSV,n,H,W,hits", default=None)
    ap.add_argument("--backward", action="store_true", help="time forward and backward of the differentiable render")
    ap.add_argument("--radii", action="store_true", help="time the view with per-surfel radii against radius 0, 1 and 3")
    ap.add_argument("--steps", nargs="+", type=int, default=[20, 200], help="--radii: map sizes in frames")
    ap.add_argument("--json", default=None, help="--radii / --projicp-window: write the figures to this file")
    ap.add_argument("--projicp-window", action="store_true",
                    help="only the plain odom='projicp' window of --radii (runs in a checkout of the parent commit too)")
    ap.add_argument("--parent-json", default=None, help="--radii: the --projicp-window figures of the parent commit")
    a = ap.parse_args()
    if a.projicp_window:
        import json
        runs = projicp_window()
        print("projicp, no layer: %s ms per step" % ", ".join("%.3f" % x for x in runs))
        if a.json:
            json.dump({"ms_per_step": runs}, open(a.json, "w"))
    elif a.radii:
        radii_times(a.steps, a.out, a.json, a.parent_json)
    elif a.backward:
        backward_times(a.out)
    elif a.trace_run:
        trace_run(a.trace_run)
    elif a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
    else:
        compare(a.out)
