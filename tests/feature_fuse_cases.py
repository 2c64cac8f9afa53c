"""Driver runs of the feature-layer tests (tests/test_hip_feature_fuse.py): the same small PointFusion sequences through
`step`, `forward`, a hand-written loop of existing calls plus ops.fuse_features_batch, and without a layer.  Also the
program of the child processes that repeat the `step` runs with GRADSLAM_HIP_FASTPATH=0:

    python -m tests.feature_fuse_cases OUT.npz
"""
import sys

import numpy as np
import torch

B, L, H, W, C = 2, 6, 24, 32, 5
ODOMS = ("gradicp", "projicp")
SCHEDULES = dict(prune_min_confidence=1.5, prune_min_age=1, prune_every=2, carve_margin=0.05, voxel_size=0.02)


def inputs(dtype):
    import gradslam_amd as gs
    from gradslam_amd.datasets.synthetic import make_sequence
    seqs = [make_sequence(L, H, W, seed=40 + b) for b in range(B)]
    st = lambda k: torch.from_numpy(np.stack([s[k] for s in seqs])).cuda()      # noqa: E731
    poses = st("poses")
    poses[:, 1:] = poses[:, :1]
    frames = gs.RGBDImages(st("colors"), st("depths"), st("intrinsics"), poses)
    g = torch.Generator().manual_seed(7)
    feats = (torch.rand((B, L, H, W, C), generator=g) * 4 - 2).to(dtype).cuda()
    valid = (torch.rand((B, L, H, W), generator=g) < 0.8).cuda()
    return frames, feats, valid


def slam_of(odom, **kw):
    import gradslam_amd as gs
    return gs.slam.PointFusion(odom=odom, dsratio=2, device="cuda", **kw)


def snapshot(pc, layer, poses):
    cat = lambda ts: np.concatenate([t.detach().cpu().numpy() for t in ts])     # noqa: E731
    out = dict(n=np.array([int(t.shape[0]) for t in pc.points_list]), pts=cat(pc.points_list), nrm=cat(pc.normals_list),
               col=cat(pc.colors_list), cc=cat(pc.features_list), poses=np.stack([p.cpu().numpy() for p in poses]))
    if layer is not None:
        out.update(emb=cat(layer.features_list), wgt=cat(layer.weights_list))
    return out


def run_steps(odom, dtype, *, layer=True, every=1, masked=False, per_step=None, **kw):
    """the step loop; features on every `every`-th frame; per_step(pc, layer, s) after every step (it may read the lists,
    which resolves the device-side counts: the next step then takes the generic path)"""
    import gradslam_amd as gs
    frames, feats, valid = inputs(dtype)
    slam = slam_of(odom, **kw)
    pc = gs.Pointclouds(device="cuda")
    lay = gs.MapFeatures(C, dtype) if layer else None
    if lay is not None:
        pc.attach_features(lay)
    prev, poses = None, []
    for s in range(L):
        live = frames[:, s]
        more = {}
        if lay is not None and s % every == 0:
            more = dict(features=feats[:, s:s + 1] if s % 2 else feats[:, s],          # (both accepted shapes)
                        features_valid=valid[:, s] if masked else None)
        pc, p = slam.step(pc, live, prev, inplace=True, **more)
        prev = live
        poses.append(p[:, 0])
        if per_step is not None:
            per_step(pc, lay, s)
    out = snapshot(pc, lay, poses)
    out["fast"] = np.array(getattr(slam, "_step_plan", None) is not None)
    return out


def run_forward(odom, dtype, *, masked=False, **kw):
    frames, feats, valid = inputs(dtype)
    pc, poses = slam_of(odom, **kw).forward(frames, features=feats, features_valid=valid if masked else None)
    assert pc.map_features is not None and pc.map_features.dtype == dtype
    return snapshot(pc, pc.map_features, [poses[:, s] for s in range(L)])


def run_hand(odom, dtype, *, every=1, masked=False):
    """the same through existing calls: the driver's localisation, ops.update_map_fusion_batch_ and, on buffers of its
    own, ops.fuse_features_batch"""
    import gradslam_amd as gs
    from gradslam_amd import ops
    from gradslam_amd.slam.fusionutils import RENORMALIZE_UNMATCHED
    frames, feats, valid = inputs(dtype)
    slam = slam_of(odom)
    pc = gs.Pointclouds(device="cuda")
    P = H * W
    emb = [torch.empty((L * P + 8, C), dtype=dtype, device="cuda") for _ in range(B)]
    wgt = [torch.empty(L * P + 8, dtype=torch.float32, device="cuda") for _ in range(B)]
    prev, poses = None, []
    for s in range(L):
        live = frames[:, s]
        live.poses = slam._localize(pc, live, prev)
        if len(pc) == 0:
            pc._init_empty_batch(B, 1)
        alpha = live._alpha_map(slam.sigma)
        maps = [ops.MapRows(*pc._reserve(b, P, pc.RESERVE_FRAMES), *pc._count_of(b)) for b in range(B)]
        depth = live.depth_image[:, 0, ..., 0]
        cnt, _, _, best = ops.update_map_fusion_batch_(
            maps, live.vertex_map[:, 0], live.normal_map[:, 0], depth, live.rgb_image[:, 0], alpha[:, 0, ..., 0],
            live.poses[:, 0].contiguous(), live.intrinsics[:, 0].contiguous(), slam.dist_th, slam.dot_th,
            RENORMALIZE_UNMATCHED)
        pc._set_counts_dev(cnt, P)
        use = s % every == 0
        r = ops.fuse_features_batch(list(zip(emb, wgt)), [(m.n_bound, m.n_dev) for m in maps], best, depth,
                                    alpha[:, 0, ..., 0], feats[:, s] if use else None,
                                    valid[:, s] if use and masked else None)
        assert torch.equal(r.counts, cnt)
        prev = live
        poses.append(live.poses[:, 0])
    out = snapshot(pc, None, poses)
    out.update(emb=np.concatenate([emb[b][:out["n"][b]].cpu().numpy() for b in range(B)]),
               wgt=np.concatenate([wgt[b][:out["n"][b]].cpu().numpy() for b in range(B)]))
    return out


def step_runs():
    """the `step` runs that are repeated without the fast path: name -> result"""
    runs = {}
    for odom in ODOMS:
        runs[odom + "_f16"] = run_steps(odom, torch.float16)
        runs[odom + "_f32_second_masked"] = run_steps(odom, torch.float32, every=2, masked=True)
        runs[odom + "_f16_schedules"] = run_steps(odom, torch.float16, **SCHEDULES)
    return runs


def flat(runs):
    return {"%s/%s" % (name, k): v for name, r in runs.items() for k, v in r.items()}


if __name__ == "__main__":
    np.savez(sys.argv[1], **flat(step_runs()))
