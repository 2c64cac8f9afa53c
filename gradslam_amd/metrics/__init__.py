"""Trajectory / map / table parity metrics of the SLAM path.

The reference ships an EMPTY `gradslam.metrics` package (gradslam/metrics/__init__.py); SURVEY.md section 5 / 8(d)
assign the reporters the parity harness needs to this build: pose ATE and RPE against a reference trajectory, the
distance between two fused maps (exact nearest neighbours through the HIP grid engine, gs_knn1_grid_f32), the number of
differing rows of two `pc2im_bnhw` correspondence tables, the per-frame drift of surfel counts, and the depth residual
between the rendered map and the frames it was built from (the reference-free consistency measure of a surfel map), as
a report (`depth_residual`) and as a loss on the autograd tape (`render_loss`).
bench.py and the parity tests import these (inputs may be torch tensors on any device or numpy arrays; only `map_chamfer`,
`depth_residual` and `render_loss` need the GPU).
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

__all__ = ["ate_rmse", "rpe", "map_chamfer", "table_parity", "count_drift", "depth_residual", "render_loss"]


def _poses(p) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(p) if not torch.is_tensor(p) else p).detach().to("cpu", torch.float64)
    if t.shape[-2:] != (4, 4):
        raise ValueError("Expected poses of shape (..., L, 4, 4). Got {0}.".format(tuple(t.shape)))
    return t


def ate_rmse(poses_a, poses_b) -> float:
    """Absolute trajectory error (the metric BASELINE.json's target `pose ATE <= 1e-4 m` is stated in):
    RMSE over frames of the translation difference of two (..., L, 4, 4) pose stacks expressed in the same world frame
    (no alignment: both trajectories start from the same given first pose)."""
    a, b = _poses(poses_a), _poses(poses_b)
    if a.shape != b.shape:
        raise ValueError("pose stacks differ in shape: {0} vs {1}".format(tuple(a.shape), tuple(b.shape)))
    d = a[..., :3, 3] - b[..., :3, 3]
    return float(torch.sqrt((d * d).sum(-1).mean()))


def _inv_rigid(T: torch.Tensor) -> torch.Tensor:
    R, t = T[..., :3, :3], T[..., :3, 3:]
    out = torch.zeros_like(T)
    out[..., :3, :3] = R.transpose(-1, -2)
    out[..., :3, 3:] = -R.transpose(-1, -2) @ t
    out[..., 3, 3] = 1.0
    return out


def rpe(poses_a, poses_b, delta: int = 1) -> Dict[str, float]:
    """Relative pose error over frame pairs (s, s + delta): with E = (A_s^-1 A_{s+delta})^-1 (B_s^-1 B_{s+delta}),
    RMSE of |trans(E)| in metres and of the rotation angle of E in radians."""
    a, b = _poses(poses_a), _poses(poses_b)
    if a.shape != b.shape:
        raise ValueError("pose stacks differ in shape: {0} vs {1}".format(tuple(a.shape), tuple(b.shape)))
    if not (isinstance(delta, int) and 0 < delta < a.shape[-3]):
        raise ValueError("delta must be an int in [1, L - 1]. Got {0}.".format(delta))
    ra = _inv_rigid(a[..., :-delta, :, :]) @ a[..., delta:, :, :]
    rb = _inv_rigid(b[..., :-delta, :, :]) @ b[..., delta:, :, :]
    E = _inv_rigid(ra) @ rb
    tr = E[..., :3, 3].norm(dim=-1)
    # angle from both the trace and the skew part (acos alone loses half the digits near zero)
    cos = ((E[..., 0, 0] + E[..., 1, 1] + E[..., 2, 2]) - 1.0) / 2.0
    sk = torch.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], -1)
    ang = torch.atan2(sk.norm(dim=-1) / 2.0, cos)
    return {"trans_rmse_m": float(torch.sqrt((tr * tr).mean())), "rot_rmse_rad": float(torch.sqrt((ang * ang).mean())),
            "trans_max_m": float(tr.max()), "rot_max_rad": float(ang.max()), "pairs": int(tr.numel())}


def _points_of(x, b: int) -> torch.Tensor:
    if hasattr(x, "points_list"):
        x = x.points_list[b]
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.ndim != 2 or t.shape[-1] != 3:
        raise ValueError("Expected an (N, 3) point array or a Pointclouds. Got shape {0}.".format(tuple(t.shape)))
    return t


def map_chamfer(map_a, map_b, batch_index: int = 0, device: Optional[torch.device] = None) -> Dict[str, float]:
    """Distance between two fused maps (Pointclouds, or (N, 3) arrays): for every point of one map the EXACT nearest
    point of the other (gs_knn1_grid_f32: the uniform-grid engine of the ICP loop, bit-identical to brute force), both
    ways.  Returns RMS / mean / max nearest-neighbour distances in metres and the symmetric chamfer distance (sum of
    the two mean squared distances).  Needs the HIP library (maps given as numpy arrays are moved to `device`)."""
    from .. import ops
    a, b = _points_of(map_a, batch_index), _points_of(map_b, batch_index)
    if device is None:
        device = a.device if a.is_cuda else (b.device if b.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    a, b = a.to(device, torch.float32).contiguous(), b.to(device, torch.float32).contiguous()
    if a.shape[0] == 0 or b.shape[0] == 0:
        raise ValueError("map_chamfer needs two non-empty maps")
    _, dab = ops.knn1_grid(a, b)
    _, dba = ops.knn1_grid(b, a)
    dab, dba = dab.double(), dba.double()
    return {"a_to_b_rms_m": float(dab.mean().sqrt()), "b_to_a_rms_m": float(dba.mean().sqrt()),
            "a_to_b_mean_m": float(dab.sqrt().mean()), "b_to_a_mean_m": float(dba.sqrt().mean()),
            "a_to_b_max_m": float(dab.max().sqrt()), "b_to_a_max_m": float(dba.max().sqrt()),
            "chamfer_m2": float(dab.mean() + dba.mean()), "points_a": int(a.shape[0]), "points_b": int(b.shape[0])}


def table_parity(table_a, table_b) -> Dict[str, object]:
    """Two `pc2im_bnhw` correspondence tables ((n, 4) int64 rows [b, n, h, w]; slam/fusionutils.py:238,342-347): rows of
    one that are missing from the other (as sets), and whether the tables are identical INCLUDING the row order the
    reference's ordering contracts fix (north_star: "correspondence / index masks bit-exact")."""
    a = torch.as_tensor(np.asarray(table_a) if not torch.is_tensor(table_a) else table_a).detach().cpu().to(torch.int64)
    b = torch.as_tensor(np.asarray(table_b) if not torch.is_tensor(table_b) else table_b).detach().cpu().to(torch.int64)
    for t in (a, b):
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("Expected (n, 4) tables. Got shape {0}.".format(tuple(t.shape)))
    identical = a.shape == b.shape and bool(torch.equal(a, b))
    if identical:
        return {"rows_a": int(a.shape[0]), "rows_b": int(b.shape[0]), "only_in_a": 0, "only_in_b": 0, "identical": True}
    both = torch.cat([a, b])
    if both.numel() and int(both.min()) < 0:
        raise ValueError("negative entries in a pc2im_bnhw table")
    rad = (both.max(0).values + 1) if both.numel() else torch.ones(4, dtype=torch.int64)
    if float(rad.double().prod()) >= 2.0 ** 62:
        raise ValueError("table entries too large to compare")

    def key(t):
        return ((t[:, 0] * rad[1] + t[:, 1]) * rad[2] + t[:, 2]) * rad[3] + t[:, 3]
    ka, kb = set(key(a).tolist()), set(key(b).tolist())
    return {"rows_a": int(a.shape[0]), "rows_b": int(b.shape[0]), "only_in_a": len(ka - kb), "only_in_b": len(kb - ka),
            "identical": False}


def count_drift(counts_a: Sequence[int], counts_b: Sequence[int]) -> Dict[str, object]:
    """Per-frame drift of the surfel counts of two runs of the same sequence (association / append decisions that went
    the other way): absolute difference per frame, its maximum, and the maximum relative to the map size."""
    a, b = np.asarray(counts_a, np.int64), np.asarray(counts_b, np.int64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("count sequences differ in shape: {0} vs {1}".format(a.shape, b.shape))
    d = np.abs(a - b)
    rel = d / np.maximum(b, 1)
    return {"per_frame": d.tolist(), "max": int(d.max()) if d.size else 0, "max_relative": float(rel.max()) if d.size else 0.0,
            "first_frame_with_drift": int(np.argmax(d > 0)) if (d > 0).any() else None}


def depth_residual(pointclouds, rgbdimages, **render_kwargs) -> Dict[str, torch.Tensor]:
    """Depth residual of a surfel map against frames: the map is rendered from every frame's pose with the frames'
    intrinsics and size (`Pointclouds.render`; render_kwargs: radius, min_confidence, cull_backfaces, radii, max_radius) and compared with
    the frame depth.  Per sequence and frame -- (B, L) float64 tensors on the host:
      coverage    pixels with a rendered depth among the pixels with a valid (> 0) frame depth
      mean_abs, median_abs, rmse   of (rendered - frame depth) over the pixels valid in both, in metres
      pixels      number of pixels valid in both
    Differences and sums are taken in float64 on the device; one host read at the end.  Frames without a pixel valid in
    both report NaN."""
    if not rgbdimages.has_poses:
        raise ValueError("depth_residual needs frames with poses")
    B, L, H, W = rgbdimages.shape
    rendered = pointclouds.render(rgbdimages.intrinsics, rgbdimages.poses, H, W, **render_kwargs)
    fd = rgbdimages.depth_image.detach()
    fd = (fd[:, :, 0] if rgbdimages.channels_first else fd[..., 0]).reshape(B, L, H * W).to(torch.float64)
    rd = rendered.depth_image[..., 0].reshape(B, L, H * W).to(torch.float64)
    valid_f, both = fd > 0, (fd > 0) & (rd > 0)
    n_f, n = valid_f.sum(-1).to(torch.float64), both.sum(-1)
    nf64 = n.to(torch.float64)
    d = torch.where(both, (rd - fd).abs(), torch.full_like(rd, float("inf")))
    dz = torch.where(both, d, torch.zeros_like(d))
    srt = d.sort(dim=-1).values   # the n valid residuals first; median = mean of the two middle ones
    lo, hi = ((n - 1).clamp(min=0) // 2).unsqueeze(-1), (n // 2).clamp(max=H * W - 1).unsqueeze(-1)
    med = 0.5 * (srt.gather(-1, lo) + srt.gather(-1, hi)).squeeze(-1)
    nan = torch.full_like(nf64, float("nan"))
    some = n > 0
    stats = torch.stack([torch.where(n_f > 0, nf64 / n_f, nan), torch.where(some, dz.sum(-1) / nf64, nan),
                         torch.where(some, med, nan), torch.where(some, ((dz * dz).sum(-1) / nf64).sqrt(), nan), nf64])
    stats = stats.cpu()
    return {"coverage": stats[0], "mean_abs": stats[1], "median_abs": stats[2], "rmse": stats[3], "pixels": stats[4]}


def render_loss(pointclouds, rgbdimages, *, depth_weight: float = 1.0, color_weight: float = 0.0,
                **render_kwargs) -> torch.Tensor:
    """Photometric / geometric consistency of a surfel map with frames, ON THE AUTOGRAD TAPE: the map is rendered from
    every frame's pose (`Pointclouds.render(differentiable=True)`; render_kwargs: radius, radii, max_radius, min_confidence,
    cull_backfaces) and compared with the frame.  Per sequence and frame -- a (B, L) float32 tensor on the device:
      depth_weight * mean of 1/2 (rendered - frame depth)^2  +  color_weight * mean of 1/2 |rendered - frame colour|^2
    both means over the pixels valid in both (rendered depth > 0 and frame depth > 0: the mask of `depth_residual`, a
    constant of the gradient), so that with the defaults the value is 1/2 rmse^2 of `depth_residual`.  A frame without
    such a pixel gives 0 and no gradient (never NaN).  Gradients reach the map buffers and the frames' poses through
    the HIP backward of the render (the winner of every pixel is a constant); the frames' own depth and colour are
    targets (detached).  Differences and sums are taken in float64 on the device, the result is rounded once."""
    if not rgbdimages.has_poses:
        raise ValueError("render_loss needs frames with poses")
    B, L, H, W = rgbdimages.shape
    rendered = pointclouds.render(rgbdimages.intrinsics, rgbdimages.poses, H, W, differentiable=True, **render_kwargs)
    fd = rgbdimages.depth_image.detach()
    fd = (fd[:, :, 0] if rgbdimages.channels_first else fd[..., 0]).reshape(B, L, H * W).to(torch.float64)
    rd = rendered.depth_image[..., 0].reshape(B, L, H * W).to(torch.float64)
    both = (fd > 0) & (rd.detach() > 0)
    n = both.sum(-1).to(torch.float64)
    inv = torch.where(n > 0, 1.0 / n.clamp(min=1.0), torch.zeros_like(n))
    zero = torch.zeros_like(rd)
    loss = torch.zeros((B, L), dtype=torch.float64, device=rd.device)
    if depth_weight:
        d = torch.where(both, rd - fd, zero)
        loss = loss + float(depth_weight) * 0.5 * (d * d).sum(-1) * inv
    if color_weight:
        fc = rgbdimages.rgb_image.detach()
        fc = (fc.permute(0, 1, 3, 4, 2) if rgbdimages.channels_first else fc).reshape(B, L, H * W, 3).to(torch.float64)
        rc = rendered.rgb_image.reshape(B, L, H * W, 3).to(torch.float64)
        c = torch.where(both.unsqueeze(-1), rc - fc, torch.zeros_like(rc))
        loss = loss + float(color_weight) * 0.5 * (c * c).sum((-1, -2)) * inv
    return loss.to(torch.float32)
