"""Projective-association ICP against the model view: what one localisation costs next to the grid-search ICP, what the
frame loop gains or loses with it, and what a launch of it costs (needs the MI355X; fails without one).

    python tools/projective_icp_profile.py [--out FILE] [--only localize|slam|launches|backward] [--steps K] [--color-weight W]
                                           [--huber-delta D] [--color-huber-delta C] [--huber-k K] [--color-huber-k K]
                                           [--parent-lib SO] [--pixel-weights ones|mask]

1. One localisation.  640x480 frames of the benchmark's synthetic sequences, the map fused from the first 10 frames under
   the ground-truth poses, frame 10 localised from the pose of frame 9; B = 1 and B = 8.
     new       ProjectiveICPOdometryProvider.localize: the render of the index image (ops.render_map_batch) + 10
               Gauss-Newton iterations (ops.projective_icp_batch), strides 4 and 1.
     baseline  ops.localize_batch on the same frames and maps: the grid-search gradICP at ds = 4 with the driver's 20
               iterations, and with 10.
   Timing: device events around `reps` back-to-back calls that end in a synchronise, the variants alternating in one
   process after a warm-up of each; median / min / max over the rounds.  Next to each time: the translation error of the
   pose against the ground truth (the variants solve different problems: this is a cost and accuracy report, not a
   parity check).

2. The frame loop.  A 20-step window of the B = 8 run at 640x480 (10 warm-up frames) with PointFusion(odom="projicp") and
   PointFusion(odom="gradicp"), both with the drivers' defaults (dsratio 4, 20 iterations): frames/s, ms per step and the
   ATE (RMSE of the translation error against the ground truth over the timed frames) of both, gradicp repeated for the
   spread of the same code.

3. Launches.  The solve alone (no render) at 10 and at 40 iterations: the slope is the time of one iteration = one
   linearise launch + one finish launch; and the render alone.  For the split between the two kernels run
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/projective_icp_profile.py --only launches
   in a run of its own (tracing slows the host: no end-to-end number comes from that run).

--color-weight W (W > 0) adds the joint geometric + photometric solve to parts 1 and 3, alternating with the plain one in
the same process: the provider with color_weight=W (render with the colour image + ops.model_intensity +
ops.projective_icp_color_batch), and in part 3 the intensity pre-pass and the colour solve alone.  The benchmark's frame
colours are per-frame noise: the times hold, the poses of these variants say nothing.

--huber-delta D (metres, D > 0) adds the solve with Huber weights to parts 1 and 3, alternating with the plain one in the
same process: the provider with huber_delta=D, and in part 3 the robust solve alone (10 and 40 iterations: the slope is
one robust linearise launch + the plain finish launch).  --color-huber-delta C (C > 0, needs --color-weight) does the
same for the joint solve with both thresholds.

--huber-k K (K > 0; 1.345 is the usual constant) adds the solve whose Huber threshold is estimated from the residuals'
median in every iteration (--huber-delta is then its floor) to all three parts, alternating with the plain and the
constant-threshold solve in the same process: the provider with huber_k=K in part 1, the scaled solve alone in part 3
(the slope is its four launches: residual pass, select, robust linearise, finish) and PointFusion(odom="projicp",
huber_k=K) in part 2 (frames/s and ATE next to the plain projicp run).

--color-huber-k K (K > 0, needs --color-weight) adds to part 3 the joint solve whose COLOUR threshold is estimated from the
colour residuals' median in every iteration (--color-huber-delta is then its floor), alternating in the same process
with the joint solve under a constant colour threshold (the one given, else 0.05) and, with --huber-k, with the joint
solve under the geometric rule alone and under both rules: us_per_iteration_color_const / _cscaled / _gscaled /
_bothscaled.  Every scaled variant has the same four launches per iteration.

4. The backward (--only backward; not part of a run without --only).  One call of ops.projective_icp_backward_batch on
   the tape of the 10-iteration solve of part 3, all four outputs asked for (vertex_bar, points_bar, normals_bar,
   init_pose_bar), strides 4 and 1, B = 1 and B = 8: the atomic mode (deterministic=False) and the ordered mode
   (deterministic=True) alternating in the same process.  ordered_extra_ms is what the record, the sort and the settle
   step add; at B = 8 it is set next to 8 x the B = 1 figure: one sort per launch group must cost less than the sorts of
   8 separate sequences.  With --parent-lib the atomic mode of that build (its gs_projective_icp_backward_batch_f32
   behind this tree's Python layer) alternates with this tree's: the default path must not have got slower.

--pixel-weights ones|mask adds the solve with per-pixel weights (ops.projective_icp_batch(pixel_weights=...), the
gs_weighted_* kernels) to part 3 and to the backward, alternating in the same process with the unweighted solves of the
same tree (and, with --parent-lib, with the parent's robust solve): solve_weighted_10it / _40it with the thresholds given
(--huber-delta, and with --huber-k also solve_weighted_scaled_*), us_per_iteration_weighted next to
us_per_iteration_robust, and in the backward weighted_atomic / weighted_ordered (pixel_weights_bar asked for) next to
atomic / ordered.  ones: every weight 1.0 (the unweighted solve's bits); mask: 1.0 with the centre block of 15 % of the
image 0 (those slots are masked: they stop at the weight).

--parent-lib SO (needs --huber-delta, or --only backward): the libgradslam_hip.so of another build of this project, e.g. of the parent commit
(same ABI version), loaded next to this tree's.  Part 3 then also times ITS gs_projective_icp_robust_batch_f32 on the
same descriptors, alternating with this tree's solves in the same process: what a change to the robust kernels cost."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640
MAP_FRAMES = 10


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def time_round_robin(torch, fns, reps, rounds):
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[key].append(e0.elapsed_time(e1) / reps)
    return {k: stats(v) for k, v in res.items()}


def scene(torch, gs, B):
    """(map fused from MAP_FRAMES frames under the ground truth, live frame, previous poses, ground truth of the live frame)"""
    import bench
    device = torch.device("cuda")
    frames, gt = bench.make_sequences_on_device(gs, list(range(B)), MAP_FRAMES + 1, H, W, device)
    gt_poses = torch.from_numpy(gt[0]["poses"]).to(device)
    frames.poses = gt_poses.unsqueeze(0).expand(B, -1, 4, 4).contiguous()
    slam = gs.slam.PointFusion(odom="gt", device=device)
    pc = gs.Pointclouds(device=device)
    for s in range(MAP_FRAMES):
        pc, _ = slam.step(pc, frames[:, s], None, inplace=True)
    live = frames[:, MAP_FRAMES]
    prev = gt_poses[MAP_FRAMES - 1].view(1, 1, 4, 4).expand(B, 1, 4, 4).contiguous()
    torch.cuda.synchronize()
    return pc, live, prev, gt_poses[MAP_FRAMES]


def translation_error(T, gt):
    return [float(x) for x in (T.reshape(-1, 4, 4)[:, :3, 3].double() - gt[:3, 3].double()).norm(dim=1).cpu()]


def localize_times(torch, gs, ops, reps=5, rounds=7, color_weight=0.0, huber_delta=0.0, color_huber_delta=0.0,
                   huber_k=0.0):
    from gradslam_amd.odometry import ProjectiveICPOdometryProvider
    out = []
    for B in (1, 8):
        pc, live, prev, gt = scene(torch, gs, B)
        fr = live.to_channels_last()
        K = fr.intrinsics[:, 0].contiguous()
        vertex, depth = fr.vertex_map[:, 0], fr.depth_image[:, 0, ..., 0]
        fr.normal_map   # (the frame maps are computed once, outside the timed region, for every variant)
        maps4 = [(pc._buf["points"][b], pc._buf["normals"][b]) + tuple(pc._count_of(b)) for b in range(B)]
        rows = pc._tighten_counts()
        prov = {s: ProjectiveICPOdometryProvider(numiters=10, stride=s) for s in (4, 1)}
        fns = {
            "projicp_stride4_10it": lambda: prov[4].localize(pc, live, prev),
            "projicp_stride1_10it": lambda: prov[1].localize(pc, live, prev),
            "gradicp_ds4_20it": lambda: ops.localize_batch(vertex, depth, K, prev[:, 0], maps4, 4, mode=1, numiters=20),
            "gradicp_ds4_10it": lambda: ops.localize_batch(vertex, depth, K, prev[:, 0], maps4, 4, mode=1, numiters=10),
        }
        if color_weight > 0:
            cprov = {s: ProjectiveICPOdometryProvider(numiters=10, stride=s, color_weight=color_weight) for s in (4, 1)}
            fns["projicp_color_stride4_10it"] = lambda: cprov[4].localize(pc, live, prev)
            fns["projicp_color_stride1_10it"] = lambda: cprov[1].localize(pc, live, prev)
        if huber_delta > 0:
            rprov = {s: ProjectiveICPOdometryProvider(numiters=10, stride=s, huber_delta=huber_delta) for s in (4, 1)}
            fns["projicp_robust_stride4_10it"] = lambda: rprov[4].localize(pc, live, prev)
            fns["projicp_robust_stride1_10it"] = lambda: rprov[1].localize(pc, live, prev)
        if huber_k > 0:
            sprov = {s: ProjectiveICPOdometryProvider(numiters=10, stride=s, huber_delta=huber_delta, huber_k=huber_k)
                     for s in (4, 1)}
            fns["projicp_scaled_stride4_10it"] = lambda: sprov[4].localize(pc, live, prev)
            fns["projicp_scaled_stride1_10it"] = lambda: sprov[1].localize(pc, live, prev)
        if color_weight > 0 and (huber_delta > 0 or color_huber_delta > 0):
            rcprov = {s: ProjectiveICPOdometryProvider(numiters=10, stride=s, color_weight=color_weight,
                                                       huber_delta=huber_delta, color_huber_delta=color_huber_delta)
                      for s in (4, 1)}
            fns["projicp_color_robust_stride4_10it"] = lambda: rcprov[4].localize(pc, live, prev)
            fns["projicp_color_robust_stride1_10it"] = lambda: rcprov[1].localize(pc, live, prev)
        err = {k: translation_error(fn(), gt) for k, fn in fns.items()}
        for fn in fns.values():
            fn(), fn()
        t = time_round_robin(torch, fns, reps, rounds)
        rec = {"B": B, "color_weight": color_weight, "huber_delta": huber_delta, "color_huber_delta": color_huber_delta,
               "huber_k": huber_k, "H": H, "W": W, "map_rows": rows, "initial_translation_error_m": translation_error(prev, gt)[0],
               "variants": {k: dict(t[k], translation_error_m=err[k]) for k in fns}}
        for s in (4, 1):
            rec["speedup_stride%d_vs_gradicp_20it" % s] = \
                t["gradicp_ds4_20it"]["median_ms"] / t["projicp_stride%d_10it" % s]["median_ms"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def parent_robust_solve(ops, parent, args, stride, numiters, huber_delta):
    """the constant-threshold robust solve of another build's library on descriptors filled by this tree's Python layer
    (the structs are part of the ABI, which both share)"""
    from gradslam_amd import _C
    opt = ops._picp_options("projective_icp", geometry=(stride, numiters, 1e-8, 0.1, 30.0))
    seqs, held, dev, Bn, Hh, Ww = ops._picp_seqs("projective_icp", *args)
    ops._picp_scratch(seqs, dev, "plain", Hh, Ww, stride)
    T, _, prm = ops._picp_outputs("projective_icp", list(seqs), dev, None, False, ops.PICP_TRACE, opt)
    st = ops.stream(dev)

    def call():
        status = parent.gs_projective_icp_robust_batch_f32(seqs, None, Bn, Hh, Ww, prm, huber_delta, st)
        assert status == 0 and held and T is not None, parent.gs_last_error()
    return call


def load_parent(path):
    import ctypes
    from gradslam_amd import _C
    parent = ctypes.CDLL(os.path.abspath(path))
    for name in ("gs_projective_icp_robust_batch_f32", "gs_projective_icp_backward_batch_f32"):
        fn = getattr(parent, name)
        fn.argtypes, fn.restype = _C._PROTOS[name], ctypes.c_int
    parent.gs_last_error.restype = ctypes.c_char_p
    if parent.gs_abi_version() != _C.ABI_VERSION:
        sys.exit("--parent-lib: ABI version %d, this tree has %d" % (parent.gs_abi_version(), _C.ABI_VERSION))
    return parent


def pixel_weights_of(torch, which, B):
    """the weight images (B, H, W) of --pixel-weights"""
    w = torch.ones((B, H, W), dtype=torch.float32, device="cuda")
    if which == "mask":     # 186 x 248 of 480 x 640: 15 % of the image
        w[:, 147:333, 196:444] = 0
    return w


def launch_times(torch, gs, ops, reps=5, rounds=7, color_weight=0.0, huber_delta=0.0, color_huber_delta=0.0,
                 huber_k=0.0, parent=None, color_huber_k=0.0, pixel_weights=None):
    out = []
    for B in (1, 8):
        pc, live, prev, _ = scene(torch, gs, B)
        wts = pixel_weights_of(torch, pixel_weights, B) if pixel_weights else None
        fr = live.to_channels_last()
        K = fr.intrinsics[:, 0].contiguous()
        maps = [(pc._buf["points"][b], None, None, None) + tuple(pc._count_of(b)) for b in range(B)]
        maps_n = [(pc._buf["points"][b], pc._buf["normals"][b]) + tuple(pc._count_of(b)) for b in range(B)]
        index = ops.render_map_batch(maps, prev, K, H, W).index[:, 0]
        args = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, index, prev[:, 0], maps_n,
                prev[:, 0])
        if color_weight > 0:
            maps_c = [(pc._buf["points"][b], None, pc._buf["colors"][b], None) + tuple(pc._count_of(b)) for b in range(B)]
            view = ops.render_map_batch(maps_c, prev, K, H, W)
            model = ops.model_intensity(view.color[:, 0], view.index[:, 0])
            cargs = args + (fr.rgb_image[:, 0].contiguous(), model)
        for stride in (4, 1):
            fns = {"render": lambda: ops.render_map_batch(maps, prev, K, H, W),
                   "solve_10it": lambda: ops.projective_icp_batch(*args, stride=stride, numiters=10),
                   "solve_40it": lambda: ops.projective_icp_batch(*args, stride=stride, numiters=40)}
            if color_weight > 0:
                kw = dict(color_weight=color_weight, stride=stride)
                fns.update({"render_with_color": lambda: ops.render_map_batch(maps_c, prev, K, H, W),
                            "model_intensity": lambda: ops.model_intensity(view.color[:, 0], view.index[:, 0]),
                            "solve_color_10it": lambda: ops.projective_icp_color_batch(*cargs, numiters=10, **kw),
                            "solve_color_40it": lambda: ops.projective_icp_color_batch(*cargs, numiters=40, **kw)})
            if huber_delta > 0:
                fns.update({"solve_robust_%dit" % n: (lambda n=n: ops.projective_icp_batch(
                    *args, stride=stride, numiters=n, huber_delta=huber_delta)) for n in (10, 40)})
            if parent is not None:
                fns.update({"solve_robust_parent_%dit" % n: parent_robust_solve(ops, parent, args, stride, n, huber_delta)
                            for n in (10, 40)})
            if huber_k > 0:
                fns.update({"solve_scaled_%dit" % n: (lambda n=n: ops.projective_icp_batch(
                    *args, stride=stride, numiters=n, huber_delta=huber_delta, huber_k=huber_k)) for n in (10, 40)})
            if wts is not None:
                fns.update({"solve_weighted_%dit" % n: (lambda n=n: ops.projective_icp_batch(
                    *args, stride=stride, numiters=n, huber_delta=huber_delta, pixel_weights=wts)) for n in (10, 40)})
                if huber_k > 0:
                    fns.update({"solve_weighted_scaled_%dit" % n: (lambda n=n: ops.projective_icp_batch(
                        *args, stride=stride, numiters=n, huber_delta=huber_delta, huber_k=huber_k, pixel_weights=wts))
                        for n in (10, 40)})
            robust_color = color_weight > 0 and (huber_delta > 0 or color_huber_delta > 0)
            if robust_color:
                fns.update({"solve_color_robust_%dit" % n: (lambda n=n: ops.projective_icp_color_batch(
                    *cargs, numiters=n, huber_delta=huber_delta, color_huber_delta=color_huber_delta, **kw))
                    for n in (10, 40)})
            # the colour threshold from the median of the colour residuals, next to what it is compared with in the same
            # round robin: the joint solve with a constant colour threshold (the one given, else 0.05) and, with
            # --huber-k, the joint solve with the geometric rule alone and with both rules
            color_scaled = {}
            if color_weight > 0 and color_huber_k > 0:
                const = color_huber_delta if color_huber_delta > 0 else 0.05
                color_scaled["color_const"] = dict(huber_delta=huber_delta, color_huber_delta=const)
                color_scaled["color_cscaled"] = dict(huber_delta=huber_delta, color_huber_delta=color_huber_delta,
                                                     color_huber_k=color_huber_k)
                if huber_k > 0:
                    color_scaled["color_gscaled"] = dict(huber_delta=huber_delta, color_huber_delta=const, huber_k=huber_k)
                    color_scaled["color_bothscaled"] = dict(huber_delta=huber_delta, color_huber_delta=color_huber_delta,
                                                            huber_k=huber_k, color_huber_k=color_huber_k)
            for name, ckw in color_scaled.items():
                fns.update({"solve_%s_%dit" % (name, n): (lambda n=n, ckw=ckw: ops.projective_icp_color_batch(
                    *cargs, numiters=n, **ckw, **kw)) for n in (10, 40)})
            for fn in fns.values():
                fn(), fn()
            t = time_round_robin(torch, fns, reps, rounds)
            per_it = (t["solve_40it"]["median_ms"] - t["solve_10it"]["median_ms"]) / 30
            nslots = -(-H // stride) * -(-W // stride)
            rec = {"B": B, "stride": stride, "slots": nslots, "chunks": -(-nslots // 256), "times": t,
                   "us_per_iteration": per_it * 1e3, "us_per_launch_mean": per_it * 1e3 / 2,
                   "us_outside_the_iterations": (t["solve_10it"]["median_ms"] - 10 * per_it) * 1e3}
            if color_weight > 0:
                rec["color_weight"] = color_weight
                rec["us_per_iteration_color"] = \
                    (t["solve_color_40it"]["median_ms"] - t["solve_color_10it"]["median_ms"]) / 30 * 1e3
            if huber_delta > 0:
                rec["huber_delta"] = huber_delta
                rec["us_per_iteration_robust"] = \
                    (t["solve_robust_40it"]["median_ms"] - t["solve_robust_10it"]["median_ms"]) / 30 * 1e3
            if parent is not None:
                rec["us_per_iteration_robust_parent"] = \
                    (t["solve_robust_parent_40it"]["median_ms"] - t["solve_robust_parent_10it"]["median_ms"]) / 30 * 1e3
            if huber_k > 0:
                rec["huber_k"] = huber_k
                rec["us_per_iteration_scaled"] = \
                    (t["solve_scaled_40it"]["median_ms"] - t["solve_scaled_10it"]["median_ms"]) / 30 * 1e3
            if wts is not None:
                rec["pixel_weights"] = pixel_weights
                rec["us_per_iteration_weighted"] = \
                    (t["solve_weighted_40it"]["median_ms"] - t["solve_weighted_10it"]["median_ms"]) / 30 * 1e3
                base = rec.get("us_per_iteration_robust_parent", rec.get("us_per_iteration_robust", rec["us_per_iteration"]))
                rec["weighted_over_" + ("robust_parent" if parent is not None else "robust" if huber_delta > 0 else "plain")] = \
                    rec["us_per_iteration_weighted"] / base
                if huber_k > 0:
                    rec["us_per_iteration_weighted_scaled"] = (t["solve_weighted_scaled_40it"]["median_ms"] -
                                                               t["solve_weighted_scaled_10it"]["median_ms"]) / 30 * 1e3
            if robust_color:
                rec["color_huber_delta"] = color_huber_delta
                rec["us_per_iteration_color_robust"] = \
                    (t["solve_color_robust_40it"]["median_ms"] - t["solve_color_robust_10it"]["median_ms"]) / 30 * 1e3
            for name in color_scaled:
                rec["color_huber_k"] = color_huber_k
                rec["us_per_iteration_" + name] = \
                    (t["solve_%s_40it" % name]["median_ms"] - t["solve_%s_10it" % name]["median_ms"]) / 30 * 1e3
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


class _BackwardOf:
    """this tree's library with the atomic backward entry of another build in its place"""

    def __init__(self, own, parent):
        self._own, self._parent = own, parent

    def __getattr__(self, name):
        return getattr(self._parent if name == "gs_projective_icp_backward_batch_f32" else self._own, name)


def backward_times(torch, gs, ops, reps=5, rounds=7, parent=None, pixel_weights=None):
    out = []
    for B in (1, 8):
        pc, live, prev, _ = scene(torch, gs, B)
        wts = pixel_weights_of(torch, pixel_weights, B) if pixel_weights else None
        fr = live.to_channels_last()
        K = fr.intrinsics[:, 0].contiguous()
        maps = [(pc._buf["points"][b], None, None, None) + tuple(pc._count_of(b)) for b in range(B)]
        maps_n = [(pc._buf["points"][b], pc._buf["normals"][b]) + tuple(pc._count_of(b)) for b in range(B)]
        index = ops.render_map_batch(maps, prev, K, H, W).index[:, 0]
        args = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, index, prev[:, 0], maps_n)
        pose_bar = torch.randn((B, 4, 4), generator=torch.Generator().manual_seed(5)).cuda()
        rows = pc._tighten_counts()
        for stride in (4, 1):
            numiters = 10
            tapes = torch.empty((B, ops.projective_icp_tape_bytes(numiters)), dtype=torch.uint8, device="cuda")
            opt = ops._picp_options("projective_icp", geometry=(stride, numiters, 1e-8, 0.1, 30.0))
            _, trace = ops._picp_solve(opt, *args, prev[:, 0], tapes=tapes, return_trace=True)

            def call(deterministic):
                return ops.projective_icp_backward_batch(*args, tapes, pose_bar, stride=stride, numiters=numiters,
                                                         deterministic=deterministic)

            def via(build, deterministic):
                """a call with the atomic entry of `build` (None: this tree's); with --parent-lib every variant goes through
                this detour, so that the host side (which is most of a call at stride 4) is the same code for all"""
                def run():
                    own = ops.lib
                    ops.lib = lambda: _BackwardOf(own(), build if build is not None else own())
                    try:
                        return call(deterministic)
                    finally:
                        ops.lib = own
                return run

            fns = {"atomic": lambda: call(False), "ordered": lambda: call(True)}
            if parent is not None:
                fns = {"atomic": via(None, False), "ordered": via(None, True), "atomic_parent": via(parent, False)}
            if wts is not None:   # the weighted backward on the weighted forward's tape, pixel_weights_bar asked for
                wtapes = torch.empty_like(tapes)
                ops._picp_solve(opt, *args, prev[:, 0], tapes=wtapes, weights=list(wts), return_trace=True)

                def wcall(deterministic):
                    return ops.projective_icp_backward_batch(*args, wtapes, pose_bar, stride=stride, numiters=numiters,
                                                             deterministic=deterministic, pixel_weights=wts,
                                                             want_pixel_weights=True)
                fns["weighted_atomic"] = lambda: wcall(False)
                fns["weighted_ordered"] = lambda: wcall(True)
            res = {k: fn() for k, fn in fns.items()}
            torch.cuda.synchronize()
            same = {k: all(torch.equal(a, b) for a, b in ((res[k][0], res["atomic"][0]), (res[k][2], res["atomic"][2])))
                    for k in fns}                                  # vertex_bar and init_pose_bar: the same bits
            # (with --pixel-weights mask the weighted variants solve another problem: their entries then read False)
            again = call(True)
            ordered_repeats = all(torch.equal(a, b) for x, y in zip(res["ordered"][1], again[1]) for a, b in zip(x, y))
            del res, again
            for fn in fns.values():
                fn(), fn()
            t = time_round_robin(torch, fns, reps, rounds)
            nslots = -(-H // stride) * -(-W // stride)
            rec = {"B": B, "stride": stride, "slots": nslots, "numiters": numiters, "map_rows": rows,
                   "inliers_last_iteration": [int(x) for x in trace[:, -1, 0].cpu()], "times": t,
                   "ordered_over_atomic": t["ordered"]["median_ms"] / t["atomic"]["median_ms"],
                   "ordered_extra_ms": t["ordered"]["median_ms"] - t["atomic"]["median_ms"],
                   "vertex_and_init_bits_equal_atomic": same, "ordered_map_gradients_repeat_bit_for_bit": ordered_repeats}
            if wts is not None:
                rec["pixel_weights"] = pixel_weights
                rec["weighted_atomic_over_atomic"] = t["weighted_atomic"]["median_ms"] / t["atomic"]["median_ms"]
                rec["weighted_ordered_over_ordered"] = t["weighted_ordered"]["median_ms"] / t["ordered"]["median_ms"]
            if parent is not None:
                a, b = t["atomic"], t["atomic_parent"]
                rec["atomic_over_parent"] = a["median_ms"] / b["median_ms"]
                rec["medians_within_each_others_spread"] = \
                    b["min_ms"] <= a["median_ms"] <= b["max_ms"] and a["min_ms"] <= b["median_ms"] <= a["max_ms"]
            print(json.dumps(rec), flush=True)
            out.append(rec)
    for stride in (4, 1):      # one sort per launch group against the sorts of 8 separate sequences
        one = next(r for r in out if r["B"] == 1 and r["stride"] == stride)
        eight = next(r for r in out if r["B"] == 8 and r["stride"] == stride)
        eight["ordered_extra_ms_of_8_single_calls"] = 8 * one["ordered_extra_ms"]
        eight["one_sort_per_group_holds"] = eight["ordered_extra_ms"] <= 8 * one["ordered_extra_ms"]
        print(json.dumps({"stride": stride, "ordered_extra_ms_B8": eight["ordered_extra_ms"],
                          "ordered_extra_ms_8_x_B1": 8 * one["ordered_extra_ms"]}), flush=True)
    return out


def slam_runs(torch, gs, steps, warmup=10, huber_delta=0.0, huber_k=0.0):
    import bench
    B = 8
    device = torch.device("cuda")
    frames, gt = bench.make_sequences_on_device(gs, list(range(B)), warmup + steps, H, W, device)
    gt_t = torch.from_numpy(gt[0]["poses"][warmup:warmup + steps, :3, 3]).to(device).double()

    def run(odom, **kw):
        slam = gs.slam.PointFusion(odom=odom, device=device, **kw)
        r = bench.timed_steps(gs, slam, frames, warmup, steps, device, lambda: torch.cuda.synchronize(device))
        e = (r["poses"][:, warmup:warmup + steps, :3, 3].double() - gt_t).norm(dim=-1)     # (B, steps)
        return {"odom": odom, "frames_per_s": B * steps / r["elapsed"], "ms_per_step": r["elapsed"] / steps * 1e3,
                "gpu_ms_per_step_median": statistics.median(r["step_ms"]),
                "ate_rmse_m": float((e * e).mean().sqrt()), "ate_max_m": float(e.max()),
                "last_frame_error_m_mean": float(e[:, -1].mean())}

    run("gradicp"), run("projicp")   # warm-up of every shape: allocator size classes, code objects
    base = run("gradicp")
    new = run("projicp")
    base2 = run("gradicp")
    out = {"B": B, "H": H, "W": W, "warmup": warmup, "steps": steps, "gradicp": base, "projicp": new,
           "gradicp_repeated": base2, "frames_per_s_ratio": new["frames_per_s"] / base["frames_per_s"]}
    if huber_k > 0:   # the median rule next to the plain projicp run, the plain one repeated for the spread
        kw = dict(huber_delta=huber_delta, huber_k=huber_k)
        run("projicp", **kw)
        out["projicp_scaled"] = dict(run("projicp", **kw), **kw)
        out["projicp_repeated"] = run("projicp")
        out["projicp_scaled_repeated"] = dict(run("projicp", **kw), **kw)
        out["frames_per_s_ratio_scaled_vs_projicp"] = out["projicp_scaled"]["frames_per_s"] / new["frames_per_s"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("localize", "slam", "launches", "backward"), default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--color-weight", type=float, default=0.0,
                    help="> 0: also time the joint geometric + photometric solve (parts 1 and 3)")
    ap.add_argument("--huber-delta", type=float, default=0.0,
                    help="> 0 (metres): also time the solve with Huber weights (parts 1 and 3)")
    ap.add_argument("--huber-k", type=float, default=0.0,
                    help="> 0: also time the solve with the Huber threshold from the residuals' median (all three parts; "
                         "--huber-delta is then its floor)")
    ap.add_argument("--parent-lib", default=None, metavar="SO",
                    help="another build's libgradslam_hip.so (needs --huber-delta): part 3 also times its robust solve")
    ap.add_argument("--color-huber-delta", type=float, default=0.0,
                    help="> 0 (intensity units, needs --color-weight): Huber weights on the colour rows of the joint solve")
    ap.add_argument("--color-huber-k", type=float, default=0.0,
                    help="> 0 (needs --color-weight): part 3 also times the joint solve with the colour Huber threshold "
                         "from the colour residuals' median (--color-huber-delta is then its floor), next to a constant "
                         "colour threshold and, with --huber-k, next to the geometric rule alone and both rules")
    ap.add_argument("--pixel-weights", choices=("ones", "mask"), default=None,
                    help="also time the solve with per-pixel weights and its backward (part 3 and --only backward), next "
                         "to the unweighted ones of the same tree")
    args = ap.parse_args()
    if not (args.color_weight >= 0 and args.color_weight < float("inf")):
        ap.error("--color-weight must be finite and not negative")
    for name in ("huber_delta", "color_huber_delta", "huber_k", "color_huber_k"):
        if not (getattr(args, name) >= 0 and getattr(args, name) < float("inf")):
            ap.error("--%s must be finite and not negative" % name.replace("_", "-"))
    if args.color_huber_delta > 0 and not args.color_weight > 0:
        ap.error("--color-huber-delta needs --color-weight")
    if args.color_huber_k > 0 and not args.color_weight > 0:
        ap.error("--color-huber-k needs --color-weight")
    if args.parent_lib and not (args.huber_delta > 0 or args.only == "backward"):
        ap.error("--parent-lib needs --huber-delta (or --only backward)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/projective_icp_profile.py measures on the GPU: no HIP device found (nothing is measured on the CPU)")
    import gradslam_amd as gs
    from gradslam_amd import ops
    out = {"device": torch.cuda.get_device_name(0)}
    if args.only in (None, "localize"):
        out["one_localisation"] = localize_times(torch, gs, ops, color_weight=args.color_weight,
                                                 huber_delta=args.huber_delta, color_huber_delta=args.color_huber_delta,
                                                 huber_k=args.huber_k)
    if args.only in (None, "slam"):
        out["slam_window"] = slam_runs(torch, gs, args.steps, huber_delta=args.huber_delta, huber_k=args.huber_k)
    if args.only in (None, "launches"):
        out["launches"] = launch_times(torch, gs, ops, color_weight=args.color_weight, huber_delta=args.huber_delta,
                                       color_huber_delta=args.color_huber_delta, huber_k=args.huber_k,
                                       color_huber_k=args.color_huber_k, parent=load_parent(args.parent_lib) if args.parent_lib else None,
                                       pixel_weights=args.pixel_weights)
    if args.only == "backward":
        out["backward"] = backward_times(torch, gs, ops, parent=load_parent(args.parent_lib) if args.parent_lib else None,
                                         pixel_weights=args.pixel_weights)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
