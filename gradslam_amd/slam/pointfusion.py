"""PointFusion driver with the reference's constructor and `_map` override
(slam/pointfusion.py:16-112): ICPSLAM odometry + surfel fusion map update."""
import math
import warnings
from typing import Optional, Union

import torch

from ..structures.mapfeatures import SurfelRadii
from ..structures.pointclouds import Pointclouds
from ..structures.rgbdimages import RGBDImages
from .fusionutils import update_map_fusion
from .icpslam import ICPSLAM

__all__ = ["PointFusion"]


class PointFusion(ICPSLAM):
    r"""Point-based Fusion (Keller et al.) on top of ICP/gradICP odometry.

    Pruning (off by default): with `prune_min_confidence` set, every `step` ends with `pointclouds.mark_epoch()`, and
    every `prune_every`-th step of a map first runs `pointclouds.prune_(prune_min_confidence, min_age=prune_min_age)`:
    surfels whose confidence count is still below the threshold `prune_min_age` steps after they were appended are
    removed (Keller et al.'s removal of points that stay unstable).  The step counter and the marks live with the map.
    With `prune_min_confidence=None` a step makes none of these calls.

    Depth pre-filter (off by default): `depth_filter=dict(radius=..., sigma_space=..., sigma_range=...)` as in `ICPSLAM`:
    the step -- fast path, generic path and `forward` alike -- works on the bilaterally filtered copy of the live frame
    and writes the recovered pose back to the caller's frame.

    Free-space carving (off by default): with `carve_margin` set, every `carve_every`-th `step` of a map ends its map
    update with `pointclouds.carve_(frame, margin=carve_margin, window=carve_window)` against the frame it just fused
    (the filtered copy when `depth_filter` is set: what was fused is what is tested) under the pose the step recovered:
    surfels the frame sees through -- something that has moved away -- are removed (Keller et al.'s free-space
    violations).  It runs before the pruning schedule, on the fast path, the generic path and `forward` alike.  With
    `carve_margin=None` a step makes no such call.

    Voxel thinning (off by default): with `voxel_size` set, every `voxel_every`-th `step` of a map follows its map
    update (and its carve) with `pointclouds.voxel_downsample_(voxel_size)`: of the surfels that share a cube of side
    `voxel_size` only the most confident stays (the oldest among equals); nothing is averaged.  It runs before the
    pruning schedule, on the fast path, the generic path and `forward` alike.  With `voxel_size=None` a step makes no
    such call.

    `odom_differentiable`: as in `ICPSLAM` (the projective ICP of `odom="projicp"` on the autograd tape).
    `color_weight`: as in `ICPSLAM` (the photometric term of `odom="projicp"`).
    `huber_delta`, `color_huber_delta`: as in `ICPSLAM` (the Huber thresholds of `odom="projicp"`).
    `huber_k`: as in `ICPSLAM` (the Huber threshold of `odom="projicp"` from the residuals' median).
    `color_huber_k`: as in `ICPSLAM` (the colour Huber threshold of `odom="projicp"` from the colour residuals' median).
    `odom_deterministic_backward`: as in `ICPSLAM` (bitwise reproducible map gradients of `odom="projicp"`'s backward).
    `odom_pixel_weights`: as in `ICPSLAM` (per-pixel weights of `odom="projicp"` from a callable on the live frame).
    `odom_outlier_mask`: as in `ICPSLAM` (the outlier mask of `odom="projicp"` and the refinement without the masked
    pixels).  `fuse_outliers` (True by default, `odom="projicp"` only): with False the pixels of that mask stay out of the
    static map: the map update of the step, and its carve, see a copy of the frame with depth 0 at the masked pixels.
    The caller's frame is untouched; the pose is written back to it as with `depth_filter`.  It needs
    `odom_outlier_mask`.

    Feature layers: on a map with a `MapFeatures` layer (`Pointclouds.attach_features`) every in-place `step` follows
    its map update with `ops.fuse_features_batch` on the update's own correspondences (a `SurfelRadii` layer makes its
    own feature image from the frame the update saw; `surfel_radii=True` has `forward` attach one and `step` insist on
    one; `odom_surfel_radii=True` renders the model view of `odom="projicp"` with it): `features` ((B, 1, H, W, C) or
    (B, H, W, C), the layer's dtype) are merged into the matched surfels with the weights of the colour fusion and
    copied to the appended ones; `features_valid` ((B, 1, H, W) or (B, H, W), bool / uint8) leaves pixels out.  A step
    without `features` still runs the pass (the appended rows are created with weight 0), so the layer never falls out
    of step with the map; it sees the frame the map update saw (`depth_filter`, `fuse_outliers=False`).  The carve, the
    thinning and the pruning schedule compact the layer with the map.  `inplace=False` with a layer raises.  `forward`
    with `features` (B, L, H, W, C) attaches a new layer (of `feature_dtype`, default: the dtype of `features`) to the
    map it builds.  There is no backward pass: a feature image that requires grad warns and the layer is detached."""

    def __init__(self, *, odom: str = "gradicp", dist_th: Union[float, int] = 0.05, angle_th: Union[float, int] = 20,
                 sigma: Union[float, int] = 0.6, dsratio: int = 4, numiters: int = 20, damp: float = 1e-8,
                 dist_thresh: Union[float, int, None] = None, lambda_max: Union[float, int] = 2.0,
                 B: Union[float, int] = 1.0, B2: Union[float, int] = 1.0, nu: Union[float, int] = 200.0,
                 device: Union[torch.device, str, None] = None, prune_min_confidence: Union[float, int, None] = None,
                 prune_min_age: int = 20, prune_every: int = 10, depth_filter: Optional[dict] = None,
                 odom_differentiable: bool = False, color_weight: Union[float, int] = 0.0,
                 huber_delta: Union[float, int] = 0.0, color_huber_delta: Union[float, int] = 0.0,
                 huber_k: Union[float, int] = 0.0, carve_margin: Union[float, int, None] = None,
                 carve_window: int = 1, carve_every: int = 1, color_huber_k: Union[float, int] = 0.0,
                 voxel_size: Union[float, int, None] = None, voxel_every: int = 1,
                 odom_deterministic_backward: Optional[bool] = None, odom_pixel_weights=None,
                 odom_outlier_mask: Optional[dict] = None, fuse_outliers: bool = True, surfel_radii: bool = False,
                 odom_surfel_radii: bool = False):
        if not isinstance(surfel_radii, bool):
            raise TypeError("surfel_radii must be of type bool; but was of type {}.".format(type(surfel_radii)))
        super().__init__(odom=odom, dsratio=dsratio, numiters=numiters, damp=damp, dist_thresh=dist_thresh,
                         lambda_max=lambda_max, B=B, B2=B2, nu=nu, device=device, depth_filter=depth_filter,
                         odom_differentiable=odom_differentiable, color_weight=color_weight, huber_delta=huber_delta,
                         color_huber_delta=color_huber_delta, huber_k=huber_k, color_huber_k=color_huber_k,
                         odom_deterministic_backward=odom_deterministic_backward,
                         odom_pixel_weights=odom_pixel_weights, odom_outlier_mask=odom_outlier_mask,
                         odom_surfel_radii=odom_surfel_radii)
        self.surfel_radii = surfel_radii
        if not isinstance(fuse_outliers, bool):
            raise TypeError("fuse_outliers must be of type bool; but was of type {}.".format(type(fuse_outliers)))
        if not fuse_outliers and odom != "projicp":
            raise ValueError("fuse_outliers is a switch of odom='projicp' (got odom={!r})".format(odom))
        if not fuse_outliers and odom_outlier_mask is None:
            raise ValueError("fuse_outliers=False needs odom_outlier_mask: it keeps the pixels of that mask out of the map")
        self.fuse_outliers = fuse_outliers
        self._fused = None      # the frame the last step's map update saw, when it was not the frame of the step
        if not (isinstance(dist_th, float) or isinstance(dist_th, int)):
            raise TypeError("Distance threshold must be of type float or int; but was of type {}.".format(
                type(dist_th)))
        if not (isinstance(angle_th, float) or isinstance(angle_th, int)):
            raise TypeError("Angle threshold must be of type float or int; but was of type {}.".format(
                type(angle_th)))
        if dist_th < 0:
            warnings.warn("Distance threshold ({}) should be non-negative.".format(dist_th))
        if not ((0 <= angle_th) and (angle_th <= 90)):
            warnings.warn("Angle threshold ({}) should be non-negative and <=90.".format(angle_th))
        self.dist_th = dist_th
        rad_th = (angle_th * math.pi) / 180
        self.dot_th = torch.cos(rad_th) if torch.is_tensor(rad_th) else math.cos(rad_th)
        self.sigma = sigma
        if not (prune_min_confidence is None or
                (isinstance(prune_min_confidence, (float, int)) and not isinstance(prune_min_confidence, bool))):
            raise TypeError("Prune confidence threshold must be of type float or int or None; but was of type {}.".format(
                type(prune_min_confidence)))
        for name, val in (("prune_min_age", prune_min_age), ("prune_every", prune_every)):
            if not isinstance(val, int) or isinstance(val, bool):
                raise TypeError("{} must be of type int; but was of type {}.".format(name, type(val)))
        if prune_min_age < 0:
            raise ValueError("prune_min_age ({}) must be non-negative.".format(prune_min_age))
        if prune_every < 1:
            raise ValueError("prune_every ({}) must be at least 1.".format(prune_every))
        if prune_min_confidence is not None and prune_min_confidence < 0:
            warnings.warn("Prune confidence threshold ({}) should be non-negative.".format(prune_min_confidence))
        if prune_min_age > Pointclouds.MAX_MARKS:
            warnings.warn("prune_min_age ({}) exceeds the {} epochs a map remembers: every surfel stays young and "
                          "nothing is pruned.".format(prune_min_age, Pointclouds.MAX_MARKS))
        self.prune_min_confidence = prune_min_confidence
        self.prune_min_age = prune_min_age
        self.prune_every = prune_every
        if not (carve_margin is None or
                (isinstance(carve_margin, (float, int)) and not isinstance(carve_margin, bool))):
            raise TypeError("Carve margin must be of type float or int or None; but was of type {}.".format(
                type(carve_margin)))
        for name, val in (("carve_window", carve_window), ("carve_every", carve_every)):
            if not isinstance(val, int) or isinstance(val, bool):
                raise TypeError("{} must be of type int; but was of type {}.".format(name, type(val)))
        if carve_margin is not None and not (0 <= carve_margin < math.inf):
            raise ValueError("carve_margin ({}) must be finite and non-negative.".format(carve_margin))
        if not 0 <= carve_window <= 3:
            raise ValueError("carve_window ({}) must be in 0..3.".format(carve_window))
        if carve_every < 1:
            raise ValueError("carve_every ({}) must be at least 1.".format(carve_every))
        self.carve_margin = carve_margin
        self.carve_window = carve_window
        self.carve_every = carve_every
        if not (voxel_size is None or (isinstance(voxel_size, (float, int)) and not isinstance(voxel_size, bool))):
            raise TypeError("Voxel size must be of type float or int or None; but was of type {}.".format(
                type(voxel_size)))
        if not isinstance(voxel_every, int) or isinstance(voxel_every, bool):
            raise TypeError("voxel_every must be of type int; but was of type {}.".format(type(voxel_every)))
        if voxel_size is not None and not (0 < voxel_size < math.inf):
            raise ValueError("voxel_size ({}) must be finite and positive.".format(voxel_size))
        if voxel_every < 1:
            raise ValueError("voxel_every ({}) must be at least 1.".format(voxel_every))
        self.voxel_size = voxel_size
        self.voxel_every = voxel_every

    def forward(self, frames: RGBDImages, *, features=None, features_valid=None, feature_dtype=None):
        r"""Returns (pointclouds: B global maps, poses (B, L, 4, 4)).  With `features` the map carries a new
        `MapFeatures` layer (`pointclouds.map_features`) fused from them frame by frame."""
        if features is None:
            if features_valid is not None or feature_dtype is not None:
                raise ValueError("features_valid / feature_dtype were given without features")
            if self.surfel_radii:
                return self._forward(frames, Pointclouds(device=self.device).attach_features(SurfelRadii()), lambda s: {})
            return super().forward(frames)
        if self.surfel_radii:
            raise ValueError("features were given, but surfel_radii=True builds a map whose one layer is a SurfelRadii")
        from ..structures.mapfeatures import MapFeatures
        if not isinstance(frames, RGBDImages):
            raise TypeError("Expected frames to be of type gradslam.RGBDImages. Got {0}.".format(type(frames)))
        B, L, H, W = frames.shape[:4]
        if not torch.is_tensor(features) or features.ndim != 5 or tuple(features.shape[:4]) != (B, L, H, W):
            raise ValueError("features must have shape ({}, {}, {}, {}, C); got {}".format(
                B, L, H, W, tuple(features.shape) if torch.is_tensor(features) else type(features)))
        if features_valid is not None and (not torch.is_tensor(features_valid) or
                                           tuple(features_valid.shape) != (B, L, H, W)):
            raise ValueError("features_valid must have shape ({}, {}, {}, {})".format(B, L, H, W))
        dtype = features.dtype if feature_dtype is None else feature_dtype
        pointclouds = Pointclouds(device=self.device).attach_features(MapFeatures(int(features.shape[-1]), dtype))
        return self._forward(frames, pointclouds, lambda s: dict(
            features=features[:, s].to(device=self.device, dtype=dtype),
            features_valid=None if features_valid is None else features_valid[:, s].to(self.device)))

    _fuses_features = True

    def _check_feature_layer(self, pointclouds):
        pass    # (PointFusion is the driver that fuses features: see step)

    def _fuse_features(self, pointclouds: Pointclouds, frame: RGBDImages, feat, valid):
        """the feature pass of a step, on the tables its map update left with the map and on the frame that update saw"""
        record, pointclouds._fuse_record = pointclouds._fuse_record, None
        if record is None:
            raise RuntimeError("the map update of this step left no correspondence table for the feature layer "
                               "(a _map override that does not go through update_map_fusion?)")
        fr = frame.to_channels_last()
        depth = fr.depth_image[:, 0, ..., 0].detach()
        alpha = fr._alpha_map(self.sigma)[:, 0, ..., 0].detach()
        if isinstance(pointclouds.map_features, SurfelRadii):
            feat, valid = pointclouds.map_features._sample(fr)
        pointclouds.map_features._fuse(pointclouds, record, depth, alpha, feat, valid)

    def step(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame=None, inplace: bool = False, *,
             features=None, features_valid=None):
        layer = pointclouds.map_features if isinstance(pointclouds, Pointclouds) else None
        feat = valid = None
        if self.surfel_radii and not isinstance(layer, SurfelRadii):
            raise ValueError("PointFusion(surfel_radii=True).step needs a map that carries a SurfelRadii layer: attach one "
                             "with pointclouds.attach_features(gradslam_amd.SurfelRadii()) before the first step (forward "
                             "does so by itself)")
        if layer is None:
            if features is not None or features_valid is not None:
                raise ValueError("features were given, but the map has no feature layer (Pointclouds.attach_features)")
        else:
            if not inplace:
                raise ValueError("a map with a feature layer is updated in place: step(..., inplace=True) (an "
                                 "out-of-place step returns a map without the layer)")
            if isinstance(live_frame, RGBDImages):
                B, L, H, W = live_frame.shape[:4]
                feat, valid = layer._frame_features(features, features_valid, B, H, W)
            pointclouds._fuse_record = None
        # the plain SLAM loop (in place, nothing on the autograd tape, a map with surfels): one foreign call per frame
        # (slam/_fastpath.py: same kernels in the same order as _localize + _map below); anything else, and every
        # subclass that overrides _localize / _map, takes the generic path
        res = None
        work = live_frame
        self._fused = None
        if self.depth_filter is not None and isinstance(live_frame, RGBDImages):
            work = self._filtered(live_frame)      # (filtered once, whichever path the step takes)
        if inplace and type(self) is PointFusion and isinstance(live_frame, RGBDImages) and \
                isinstance(prev_frame, RGBDImages) and isinstance(pointclouds, Pointclouds):
            from ._fastpath import try_step
            res = try_step(self, pointclouds, work, prev_frame)
        if res is None:
            res = super().step(pointclouds, live_frame, prev_frame, inplace) if work is live_frame else \
                self._step(pointclouds, work, prev_frame, inplace)
        if work is not live_frame:
            live_frame.poses = work.poses
        if layer is not None:
            # before the carve, the thinning and the pruning schedule: they compact the layer with the map
            self._fuse_features(res[0], work if self._fused is None else self._fused, feat, valid)
        if self.carve_margin is not None or self.voxel_size is not None or self.prune_min_confidence is not None:
            if res[0] is not pointclouds:
                # an out-of-place step returns a new container: it takes the marks and the step counters once, before
                # the carve, whose compaction rewrites the marks that the pruning schedule then reads
                res[0]._carry_epochs(pointclouds)
            if self.carve_margin is not None:
                self._carve_step(res[0], work if self._fused is None else self._fused)
            if self.voxel_size is not None:
                self._voxel_step(res[0])
            if self.prune_min_confidence is not None:
                self._end_step(res[0])
        return res

    def _step(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame, inplace: bool):
        if self.fuse_outliers:
            return super()._step(pointclouds, live_frame, prev_frame, inplace)
        # the outlier mask of this step's localisation (None when none ran: the first frame of a map) stays out of the
        # map: the update sees a copy of the frame without depth there, which carries the recovered pose
        self.odomprov.last_outlier_mask = None
        live_frame.poses = self._localize(pointclouds, live_frame, prev_frame)
        mask = self.odomprov.last_outlier_mask
        fused = live_frame if mask is None else live_frame.masked_depth(mask)
        self._fused = None if mask is None else fused
        return self._map(pointclouds, fused, inplace), live_frame.poses

    def _carve_step(self, pointclouds: Pointclouds, frame: RGBDImages):
        """free-space carving of a step (fast and generic path alike): on every carve_every-th step of this map, remove
        the surfels that the frame just fused (`frame`: the filtered copy with depth_filter; it carries the recovered
        pose) sees through"""
        pointclouds._carve_steps += 1
        if pointclouds._carve_steps % self.carve_every == 0:
            pointclouds.carve_(frame, margin=self.carve_margin, window=self.carve_window, min_views=1)

    def _voxel_step(self, pointclouds: Pointclouds):
        """voxel thinning of a step (fast and generic path alike): on every voxel_every-th step of this map, keep one
        surfel per voxel; after the carve (what the frame sees through does not compete) and before the pruning
        schedule (which reads the marks this compaction rewrites)"""
        pointclouds._voxel_steps += 1
        if pointclouds._voxel_steps % self.voxel_every == 0:
            pointclouds.voxel_downsample_(self.voxel_size)

    def _end_step(self, pointclouds: Pointclouds):
        """the pruning schedule of a step (fast and generic path alike): prune on every prune_every-th step of this map,
        then record the epoch.  The prune comes first, so that min_age = k protects the rows of the last k steps."""
        pointclouds._prune_steps += 1
        if pointclouds._prune_steps % self.prune_every == 0:
            pointclouds.prune_(self.prune_min_confidence, min_age=self.prune_min_age)
        pointclouds.mark_epoch()

    def _localize(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_frame: RGBDImages):
        if isinstance(live_frame, RGBDImages):
            # the fusion step needs the sample confidences exp(-|v|^2 / 2 sigma^2): have the kernel that
            # builds the vertex / normal maps of this frame emit them in the same pass
            live_frame._sigma_hint = float(self.sigma)
        return super()._localize(pointclouds, live_frame, prev_frame)

    def _map(self, pointclouds: Pointclouds, live_frame: RGBDImages, inplace: bool = False):
        return update_map_fusion(pointclouds, live_frame, self.dist_th, self.dot_th, self.sigma, inplace)
