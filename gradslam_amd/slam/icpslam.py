"""ICPSLAM driver with the reference's constructor, `forward`, `step`, `_localize`, `_map`
(slam/icpslam.py:18-264).  `_localize` keeps the reference's data flow (live frame back-projected
under the previous pose, map points active in the previous frame on the ds lattice as ICP target,
T_icp composed with the previous pose) but runs it as: gs_project_map_f32 ->
gs_select_targets_f32 -> gs_downsample_frame_f32 -> gs_icp_f32 (20 LM iterations + compose on
the device, no host sync inside)."""
import warnings
from typing import Optional, Union

import torch
import torch.nn as nn

from ..odometry.gradicp import GradICPOdometryProvider
from ..odometry.icp import ICPOdometryProvider
from ..odometry.projicp import ProjectiveICPOdometryProvider
from ..structures.pointclouds import Pointclouds
from ..structures.rgbdimages import RGBDImages
from .fusionutils import update_map_aggregate

__all__ = ["ICPSLAM"]


class ICPSLAM(nn.Module):
    r"""Point-to-plane ICP odometry + aggregate mapping (every valid pixel is appended).

    Depth pre-filter (off by default): with `depth_filter=dict(radius=..., sigma_space=..., sigma_range=...)` (any
    subset of the keys; the rest take the defaults of `RGBDImages.bilateral_filter`) every `step` works on the
    bilaterally filtered copy of the live frame -- localisation and map update alike -- and writes the recovered pose
    back to the caller's frame.  `prev_frame` is only read for its poses and is not filtered.  With `depth_filter=None`
    a step makes no new call.

    `odom_differentiable` (off by default, `odom="projicp"` only): the projective ICP runs on the autograd tape
    (`ProjectiveICPOdometryProvider(differentiable=True)`): the poses of `forward` and of `step` carry a `grad_fn`, and a
    loss on them reaches the depth of the frames, the initial pose and a map that requires grad.  With it off the poses
    are detached, bit for bit what they are with it on.

    `color_weight` (0 by default, `odom="projicp"` only): weight of the photometric term of the projective ICP in metres
    per intensity unit (`ProjectiveICPOdometryProvider(color_weight=...)`); the map must then carry colours.

    `huber_delta`, `color_huber_delta` (0 by default, `odom="projicp"` only): Huber thresholds of the projective ICP's
    point-to-plane residual (metres) and colour residual (intensity units; needs `color_weight`), as in
    `ProjectiveICPOdometryProvider`.

    `huber_k` (0 by default, `odom="projicp"` only): the geometric Huber threshold from the residuals' median in every
    iteration, `huber_delta` its floor (`ProjectiveICPOdometryProvider(huber_k=...)`).

    `color_huber_k` (0 by default, `odom="projicp"` only; needs `color_weight`): the colour Huber threshold from the
    colour residuals' median in every iteration, `color_huber_delta` its floor
    (`ProjectiveICPOdometryProvider(color_huber_k=...)`).

    `odom_deterministic_backward` (None by default, `odom="projicp"` only; it matters with `odom_differentiable`): True
    makes the map gradients of the projective ICP's backward bitwise reproducible, False keeps the float64 atomics, None
    follows GRADSLAM_HIP_DETERMINISTIC_BACKWARD when the backward runs
    (`ProjectiveICPOdometryProvider(deterministic_backward=...)`).

    `odom_pixel_weights` (None by default, `odom="projicp"` only): a callable that takes the live `RGBDImages` the solve
    sees (the filtered copy with `depth_filter`) and returns per-pixel weights (B, H, W) or (B, 1, H, W) for the
    projective ICP (`ProjectiveICPOdometryProvider(pixel_weights=...)`): a mask, a sensor model
    (`odometry.axial_noise_weights`), a learned confidence.  It is called once per localisation; the map update does not
    see it.  With `odom_differentiable` its output stays on the autograd tape.

    `odom_outlier_mask` (None by default, `odom="projicp"` only): a dict of the outlier mask's parameters
    (`ProjectiveICPOdometryProvider(outlier_mask=...)`: hi, lo, floor, min_support, grow, grow_depth, refine_iters, any
    subset): after the configured solve the outlier regions of the live frame are masked and refine_iters more
    iterations run without them.  The mask of the last localisation is `odomprov.last_outlier_mask`.

    `odom_surfel_radii` (False by default, `odom="projicp"` only): the model view of the projective ICP is rendered with
    the radii of the map's `SurfelRadii` layer (`ProjectiveICPOdometryProvider(surfel_radii=True)`).  Only a driver that
    fuses feature layers can keep such a map: `PointFusion` takes it, `ICPSLAM` itself raises at construction."""

    _fuses_features = False   # (ICPSLAM.step refuses a map with a feature layer: see _check_feature_layer)

    def __init__(self, *, odom: str = "gradicp", dsratio: int = 4, numiters: int = 20, damp: float = 1e-8,
                 dist_thresh: Union[float, int, None] = None, lambda_max: Union[float, int] = 2.0,
                 B: Union[float, int] = 1.0, B2: Union[float, int] = 1.0, nu: Union[float, int] = 200.0,
                 device: Union[torch.device, str, None] = None, depth_filter: Optional[dict] = None,
                 odom_differentiable: bool = False, color_weight: Union[float, int] = 0.0,
                 huber_delta: Union[float, int] = 0.0, color_huber_delta: Union[float, int] = 0.0,
                 huber_k: Union[float, int] = 0.0, color_huber_k: Union[float, int] = 0.0,
                 odom_deterministic_backward: Optional[bool] = None, odom_pixel_weights=None,
                 odom_outlier_mask: Optional[dict] = None, odom_surfel_radii: bool = False):
        super().__init__()
        from .. import ops
        if not isinstance(odom_surfel_radii, bool):
            raise TypeError("odom_surfel_radii must be of type bool; but was of type {}.".format(type(odom_surfel_radii)))
        if odom_surfel_radii and odom != "projicp":
            raise ValueError("odom_surfel_radii is a switch of odom='projicp' (got odom={!r})".format(odom))
        if odom_surfel_radii and not self._fuses_features:
            raise ValueError("odom_surfel_radii needs a map with a SurfelRadii layer, and {}.step is not supported on a "
                             "map with a feature layer attached: only PointFusion fuses features".format(
                                 type(self).__name__))
        self.odom_surfel_radii = odom_surfel_radii
        if odom_pixel_weights is not None and not callable(odom_pixel_weights):
            raise TypeError("odom_pixel_weights must be None or a callable (live frame -> weights); but was of type "
                            "{}.".format(type(odom_pixel_weights)))
        if odom_pixel_weights is not None and odom != "projicp":
            raise ValueError("odom_pixel_weights are the per-pixel weights of odom='projicp' (got odom={!r})".format(odom))
        # (not an attribute of the module: a weight network is registered by whoever owns it, the provider holds it)
        ops._picp_deterministic(type(self).__name__, "odom_deterministic_backward", odom_deterministic_backward)
        if odom_deterministic_backward is not None and odom != "projicp":
            raise ValueError("odom_deterministic_backward is a switch of odom='projicp' (got odom={!r}): the backward of "
                             "'icp' and 'gradicp' follows GRADSLAM_HIP_DETERMINISTIC_BACKWARD".format(odom))
        self.odom_deterministic_backward = odom_deterministic_backward
        ops._picp_color_weight(color_weight)
        if color_weight > 0 and odom != "projicp":
            raise ValueError("color_weight is the photometric term of odom='projicp' (got odom={!r})".format(odom))
        self.color_weight = color_weight
        for name, val in (("huber_delta", huber_delta), ("color_huber_delta", color_huber_delta)):
            ops._picp_huber(name, val, type(self).__name__)
            if val > 0 and odom != "projicp":
                raise ValueError("{} is a Huber threshold of odom='projicp' (got odom={!r})".format(name, odom))
        self.huber_delta = huber_delta
        self.color_huber_delta = color_huber_delta
        ops._picp_huber_k(huber_k, type(self).__name__)
        if huber_k > 0 and odom != "projicp":
            raise ValueError("huber_k is the Huber scale rule of odom='projicp' (got odom={!r})".format(odom))
        self.huber_k = huber_k
        ops._picp_color_huber_k(color_huber_k, type(self).__name__)
        if color_huber_k > 0 and odom != "projicp":
            raise ValueError("color_huber_k is the colour Huber scale rule of odom='projicp' (got odom={!r})".format(odom))
        self.color_huber_k = color_huber_k
        if not isinstance(odom_differentiable, bool):
            raise TypeError("odom_differentiable must be of type bool; but was of type {}.".format(
                type(odom_differentiable)))
        if odom_differentiable and odom != "projicp":
            raise ValueError("odom_differentiable is the switch of odom='projicp' (got odom={!r}): 'icp' and 'gradicp' "
                             "go on the autograd tape by themselves when an input requires grad".format(odom))
        self.odom_differentiable = odom_differentiable
        self.depth_filter = _check_depth_filter(depth_filter)
        if odom not in ["gt", "icp", "gradicp", "projicp"]:
            msg = "odometry method ({}) not supported for PointFusion. ".format(odom)
            msg += "Currently supported odometry modules for PointFusion are: 'gt', 'icp', 'gradicp', 'projicp'"
            raise ValueError(msg)
        odomprov = None
        if odom == "icp":
            odomprov = ICPOdometryProvider(numiters, damp, dist_thresh)
        elif odom == "gradicp":
            odomprov = GradICPOdometryProvider(numiters, damp, dist_thresh, lambda_max, B, B2, nu)
        elif odom == "projicp":
            # frame-to-model tracking against the rendered map: dsratio is the lattice stride, dist_thresh=None the
            # provider's 0.1 m (the gate is part of the association, it cannot be switched off)
            odomprov = ProjectiveICPOdometryProvider(numiters, damp, 0.1 if dist_thresh is None else dist_thresh,
                                                     stride=dsratio, differentiable=odom_differentiable,
                                                     color_weight=color_weight, huber_delta=huber_delta,
                                                     color_huber_delta=color_huber_delta, huber_k=huber_k,
                                                     color_huber_k=color_huber_k,
                                                     deterministic_backward=odom_deterministic_backward,
                                                     pixel_weights=odom_pixel_weights,
                                                     outlier_mask=odom_outlier_mask,
                                                     **(dict(surfel_radii=True) if odom_surfel_radii else {}))
        if odom != "projicp":
            # (checked after every other keyword, as the provider does: today's refusals and their order stay)
            ProjectiveICPOdometryProvider._outlier_mask(odom_outlier_mask)
            if odom_outlier_mask is not None:
                raise ValueError("odom_outlier_mask is the outlier mask of odom='projicp' (got odom={!r})".format(odom))
        self.odom = odom
        self.odomprov = odomprov
        self.dsratio = dsratio
        device = torch.device(device) if device is not None else torch.device("cpu")
        self.device = torch.Tensor().to(device).device

    def forward(self, frames: RGBDImages):
        r"""Returns (pointclouds: B global maps, poses (B, L, 4, 4))."""
        return self._forward(frames, Pointclouds(device=self.device), lambda s: {})

    def _forward(self, frames: RGBDImages, pointclouds: Pointclouds, step_kwargs):
        """the frame loop of `forward` into the given (empty) map; step_kwargs(s): further keywords of step s"""
        if not isinstance(frames, RGBDImages):
            raise TypeError("Expected frames to be of type gradslam.RGBDImages. Got {0}.".format(type(frames)))
        batch_size, seq_len = frames.shape[:2]
        recovered_poses = torch.empty(batch_size, seq_len, 4, 4).to(self.device)
        prev_frame = None
        for s in range(seq_len):
            live_frame = frames[:, s].to(self.device)
            if s == 0 and live_frame.poses is None:
                live_frame.poses = (torch.eye(4, dtype=torch.float, device=self.device).view(1, 1, 4, 4)
                                    .repeat(batch_size, 1, 1, 1))
            pointclouds, live_frame.poses = self.step(pointclouds, live_frame, prev_frame, inplace=True, **step_kwargs(s))
            prev_frame = live_frame if self.odom != "gt" else None
            recovered_poses[:, s] = live_frame.poses[:, 0]
        return pointclouds, recovered_poses

    def step(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame: Optional[RGBDImages] = None,
             inplace: bool = False):
        if not isinstance(live_frame, RGBDImages):
            raise TypeError("Expected live_frame to be of type gradslam.RGBDImages. Got {0}.".format(
                type(live_frame)))
        self._check_feature_layer(pointclouds)
        if self.depth_filter is None:
            return self._step(pointclouds, live_frame, prev_frame, inplace)
        work = self._filtered(live_frame)
        res = self._step(pointclouds, work, prev_frame, inplace)
        live_frame.poses = work.poses
        return res

    def _check_feature_layer(self, pointclouds):
        """the aggregate map update appends rows that no feature layer follows (PointFusion overrides this)"""
        if isinstance(pointclouds, Pointclouds) and pointclouds.map_features is not None:
            raise ValueError("ICPSLAM.step is not supported on a map with a feature layer attached: only PointFusion "
                             "fuses features (detach_features() first)")

    def _step(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame: Optional[RGBDImages], inplace: bool):
        """localise and map on the frame as given (`step` hands over the filtered copy when `depth_filter` is set)"""
        live_frame.poses = self._localize(pointclouds, live_frame, prev_frame)
        pointclouds = self._map(pointclouds, live_frame, inplace)
        return pointclouds, live_frame.poses

    def _filtered(self, live_frame: RGBDImages):
        """the frame a step works on: the live frame itself, or its bilaterally filtered copy (`depth_filter`)"""
        if self.depth_filter is None:
            return live_frame
        return live_frame.bilateral_filter(**self.depth_filter)

    def _localize(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame: RGBDImages):
        if not isinstance(pointclouds, Pointclouds):
            raise TypeError("Expected pointclouds to be of type gradslam.Pointclouds. Got {0}.".format(
                type(pointclouds)))
        if not isinstance(live_frame, RGBDImages):
            raise TypeError("Expected live_frame to be of type gradslam.RGBDImages. Got {0}.".format(
                type(live_frame)))
        if not isinstance(prev_frame, (RGBDImages, type(None))):
            raise TypeError("Expected prev_frame to be of type gradslam.RGBDImages or None. Got {0}.".format(
                type(prev_frame)))
        if prev_frame is not None:
            if self.odom == "gt":
                warnings.warn("`prev_frame` is not used when using `odom='gt'` (should be None)")
            elif not prev_frame.has_poses:
                raise ValueError("`prev_frame` should have poses, but did not.")
        if prev_frame is None and pointclouds.has_points and self.odom != "gt":
            warnings.warn("`prev_frame` was None despite `{}` odometry method. Using `live_frame` poses.".format(
                self.odom))
        if prev_frame is None or self.odom == "gt":
            if not live_frame.has_poses:
                raise ValueError("`live_frame` must have poses when `prev_frame` is None or `odom='gt'`.")
            return live_frame.poses

        if self.odom == "projicp":
            # the model view at the previous pose is target and initial guess; without odom_differentiable the result is
            # detached (a requires-grad input warns)
            return self.odomprov.localize(pointclouds, live_frame, prev_frame.poses[:, :1])

        if self.odom in ["icp", "gradicp"]:
            from .. import ops
            live_frame.poses = prev_frame.poses  # initial guess: the live frame sits at the previous pose
            fr = live_frame.to_channels_last()
            B, _, H, W = fr.shape
            K = prev_frame.intrinsics[:, 0].contiguous().float()
            prev_poses = prev_frame.poses[:, 0].contiguous().float()
            src_pts, tgt_pts, tgt_nrm = [], [], []
            # on the autograd tape whenever the reference's graph would be: the live depth, the previous pose or the
            # map (points / normals) requires grad -- for BOTH solvers (the hard-LM ICP back-propagates through its
            # accepted steps, gs_icp_backward_f32 mode 0)
            builtin = type(self.odomprov) in (ICPOdometryProvider, GradICPOdometryProvider)
            taped = torch.is_grad_enabled() and builtin and (
                fr.depth_image.requires_grad or prev_frame.poses.requires_grad or _map_requires_grad(pointclouds))
            if not taped and builtin:
                # fast path: no host read-back and no compaction of the source set.  The ICP source is the
                # frame's [::ds, ::ds] lattice of global vertices under the previous pose (NaN = no depth,
                # skipped by the solver), built from the LOCAL vertex map in one launch; the size of the
                # target set stays on the device.
                # All sequences of the batch go through ONE chain of launches (gs_localize_batch_f32).
                out = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=fr.device)
                maps = pointclouds._map_rows(("points", "normals"))
                if all(m.n_bound > 0 for m in maps):
                    ops.localize_batch(fr.vertex_map[:, 0], fr.depth_image[:, 0, ..., 0], K, prev_poses, maps,
                                       self.dsratio, mode=self.odomprov._mode, out=out.view(B, 4, 4),
                                       **self.odomprov._kwargs())
                    return out
            gvm = fr.global_vertex_map
            for b in range(B):
                # downsample_rgbdimages(live_frame): valid lattice pixels of the global vertex map
                if taped and gvm.requires_grad:
                    p = ops.DownsampleFramePointsFunction.apply(gvm[b, 0], fr.depth_image[b, 0, ..., 0].detach(),
                                                                self.dsratio)
                else:
                    p, _, _ = ops.downsample_frame(gvm[b, 0], None, None, fr.depth_image[b, 0, ..., 0], self.dsratio)
                src_pts.append(p)
                # find_active_map_points(pointclouds, prev_frame) + downsample_pointclouds, without tables
                P, N = pointclouds.points_list[b], pointclouds.normals_list[b]
                pix = ops.project_map(P, prev_poses[b], K[b], H, W)
                if taped and (P.requires_grad or N.requires_grad):
                    # the map is on the tape (differentiable mapping): gather the targets by row index so that the
                    # pose gradient also reaches the earlier frames through the map (same rows, same order)
                    rows = ops.active_table(pix, W)
                    idx = rows[(rows[:, 2] % self.dsratio == 0) & (rows[:, 3] % self.dsratio == 0), 1]
                    tp, tn = P[idx], N[idx]
                else:
                    tp, tn, _ = ops.select_targets(pix, W, self.dsratio, P, N)
                tgt_pts.append(tp)
                tgt_nrm.append(tn)
            if taped:
                # differentiable pose path: depth -> vertex -> global vertex -> ICP source -> (grad)ICP -> pose, and,
                # when the map is on the tape, earlier frames -> map -> ICP targets / normals -> pose.
                out = []
                for b in range(B):
                    T, _ = ops.grad_icp(src_pts[b], tgt_pts[b], tgt_nrm[b], None, mode=self.odomprov._mode,
                                        **self.odomprov._kwargs())
                    out.append(T)
                return _compose(torch.stack(out), prev_poses).unsqueeze(1)
            maps_pc = Pointclouds(points=tgt_pts, normals=tgt_nrm)
            frames_pc = Pointclouds(points=src_pts)
            if isinstance(self.odomprov, ICPOdometryProvider):
                # compose_transformations(T, prev_pose) fused into the last ICP kernel
                return self.odomprov.provide(maps_pc, frames_pc, compose_with=prev_poses)
            transform = self.odomprov.provide(maps_pc, frames_pc)  # user-supplied OdometryProvider plugin
            return _compose(transform.squeeze(1), prev_poses).unsqueeze(1)

    def _map(self, pointclouds: Pointclouds, live_frame: RGBDImages, inplace: bool = False):
        return update_map_aggregate(pointclouds, live_frame, inplace)


def _check_depth_filter(depth_filter):
    """None, or the complete keyword dict of RGBDImages.bilateral_filter (type and value checks of the constructor)."""
    if depth_filter is None:
        return None
    if not isinstance(depth_filter, dict):
        raise TypeError("depth_filter must be of type dict or None; but was of type {}.".format(type(depth_filter)))
    full = dict(radius=3, sigma_space=2.0, sigma_range=0.03)
    unknown = sorted(set(depth_filter) - set(full), key=str)
    if unknown:
        raise ValueError("depth_filter has unknown keys {}; expected a subset of {}.".format(unknown, sorted(full)))
    full.update(depth_filter)
    from .. import ops
    ops._bilateral_args(**full)      # (the type and value checks of ops.bilateral_depth)
    return full


def _map_requires_grad(pointclouds):
    bufs = pointclouds._buf
    return any(bufs[k] is not None and any(t.requires_grad for t in bufs[k]) for k in ("points", "normals"))


def _compose(trans_01, trans_12):
    """kornia compose_transformations for plugin providers (4x4 plumbing on the device)."""
    out = torch.zeros_like(trans_01)
    out[..., :3, :3] = trans_01[..., :3, :3] @ trans_12[..., :3, :3]
    out[..., :3, 3:] = trans_01[..., :3, :3] @ trans_12[..., :3, 3:] + trans_01[..., :3, 3:]
    out[..., 3, 3] = 1.0
    return out
