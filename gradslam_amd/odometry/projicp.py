"""ProjectiveICPOdometryProvider: frame-to-model tracking by projective data association (Keller et al., KinectFusion;
the reference has no counterpart).  The map is rendered at the previous pose (gs_render_map_dc_f32), every lattice pixel
of the live frame is paired with the surfel that won the pixel it projects to under the current estimate, and
point-to-plane Gauss-Newton steps with constant damping follow (gs_projective_icp_batch_f32) -- no nearest-neighbour
search.  The result is detached unless `differentiable` is set: the poses are then on the autograd tape
(ops.ProjectiveICPFunction, a HIP backward through the Gauss-Newton iterations).  With `color_weight` > 0 the solve
is the joint geometric + photometric one (gs_projective_icp_color_batch_f32): the view's colour image is rendered too and
the live frame's colour is compared with it.  `huber_delta` / `color_huber_delta` > 0 switch on Huber weights
(the *_robust_* entry points): rows with a large residual are down-weighted instead of pulling the pose at full weight.
`huber_k` > 0 estimates the geometric threshold from the residuals in every iteration (the *_scaled_* entry points),
`color_huber_k` > 0 the colour threshold from the colour residuals (the *_joint_scaled_* entry points).  `pixel_weights`
hands every solve a weight image made from the live frame (the *_weighted_* entry points); `axial_noise_weights` is a
ready-made one.  `outlier_mask` derives such a mask from the solve itself (gs_picp_outliers.hip): the outlier regions of
the converged solve are masked and a few more iterations run without them."""
from typing import Callable, Optional, Union

import torch

from ..structures.pointclouds import Pointclouds
from ..structures.rgbdimages import RGBDImages
from .base import OdometryProvider

__all__ = ["ProjectiveICPOdometryProvider", "axial_noise_weights"]


def axial_noise_weights(frames: RGBDImages, sigma0: float = 0.0012, k: float = 0.0019, z0: float = 0.4) -> torch.Tensor:
    r"""Per-pixel weights 1 / sigma^2(z) of a structured-light sensor's axial noise, normalised to 1 at z = z0:
    (sigma0 / (sigma0 + k (z - z0)^2))^2 with z the depth in metres, and 0 where there is no depth.  Returns
    (B, L, H, W) float32 for frames of shape (B, L, H, W): with one frame per sequence, what
    `ProjectiveICPOdometryProvider(pixel_weights=...)` expects.  Plain torch, hence differentiable in the depth.

    The defaults sigma(z) = 0.0012 + 0.0019 (z - 0.4)^2 are the published Kinect v1 axial-noise constants (Nguyen, Izadi
    and Lovell, "Modeling Kinect Sensor Noise for Improved 3D Reconstruction and Tracking", 3DIMPVT 2012); they are not
    tuned here."""
    if not isinstance(frames, RGBDImages):
        raise TypeError("Expected frames to be of type gradslam.RGBDImages. Got {0}.".format(type(frames)))
    for name, val in (("sigma0", sigma0), ("k", k), ("z0", z0)):
        if isinstance(val, bool) or not isinstance(val, (float, int)):
            raise TypeError("axial_noise_weights: {} must be of type float or int; but was of type {}.".format(
                name, type(val)))
    if not sigma0 > 0 or not k >= 0:
        raise ValueError("axial_noise_weights: sigma0 ({}) must be positive and k ({}) not negative.".format(sigma0, k))
    z = frames.to_channels_last().depth_image[..., 0].float()
    w = (sigma0 / (sigma0 + k * (z - z0) ** 2)) ** 2
    return torch.where(z > 0, w, torch.zeros_like(w))


class ProjectiveICPOdometryProvider(OdometryProvider):
    r"""Projective-association point-to-plane ICP against the model view.

    Args:
        numiters: Gauss-Newton iterations
        damp: constant damping added to the diagonal of the normal equations (> 0)
        dist_thresh: a pair is used when the transformed live vertex is within this many metres of the surfel ...
        angle_thresh: ... and their normals are within this many degrees (0..90)
        stride: the live frame's [::stride, ::stride] lattice is the source set (None: every pixel)
        min_confidence, radius: forwarded to the render of the model view (`Pointclouds.render`)
        differentiable: `localize` returns poses on the autograd tape: gradients reach the live frame's vertex map (and
            through the frame maps its depth), `prev_poses` as the initial estimate, and the map's points and normals
            where they require grad.  The association is hard and a constant of the gradient; the render that yields
            the index image stays non-differentiable (`prev_poses` as the pose of the model view gets no gradient).
            The backward pass re-reads the map rows, so run it before the map is changed in place (a
            non-differentiable in-place `step`, `prune_`); a backward after such a change raises instead of returning
            gradients of the wrong rows.  A map update that itself ran on the tape hands the map new tensors and
            leaves the saved ones intact: the backward of a loss over several such frames works.
        color_weight: weight of the photometric term in metres per intensity unit (0, the default: the geometric solve,
            bit for bit).  With a weight the map must have colours, and the live frame's `rgb_image` is read in the units
            the map's colours are stored in: for colours in 0 ... 255 start from the weight that suits [0, 1] divided by
            255.  It has no backward pass yet: a weight together with `differentiable=True` raises.
        huber_delta: Huber threshold of the point-to-plane residual in metres (0, the default: off, the plain solve bit
            for bit).  A used pair whose residual b exceeds it gets the weight huber_delta / |b|.  Works with
            `differentiable=True`.
        color_huber_delta: Huber threshold of the colour residual in the intensity units of the map's colours (0: off);
            needs `color_weight` > 0.
        huber_k: the geometric Huber threshold from the residuals themselves (0, the default: off): in every iteration
            delta = max(huber_k * 1.4826 * median|b|, huber_delta) over the used pairs, so `huber_delta` becomes a floor
            and no threshold has to be tuned per dataset; 1.345 is the usual constant.  Works with `differentiable=True`
            (the thresholds are constants of the backward pass) and with `color_weight` (without `color_huber_k` the
            colour threshold stays the constant `color_huber_delta`).
        color_huber_k: the colour Huber threshold from the colour residuals themselves (0, the default: off): in every
            iteration cdelta = max(color_huber_k * 1.4826 * median|r|, color_huber_delta) over the pairs with a colour
            row, r the colour residual before `color_weight` is applied; `color_huber_delta` becomes a floor.  The
            threshold is in the residuals' own units, so the same constant serves colours in 0 ... 1 and in 0 ... 255;
            1.345 is the usual constant.  Needs `color_weight` > 0; combines with `huber_delta` and `huber_k`.
        deterministic_backward: with `differentiable`, how the backward pass adds up the gradients of the map's points and
            normals: True = in a fixed order (bitwise reproducible, slower: the ordered mode of
            `ops.projective_icp_backward_batch`), False = float64 atomics, None (the default) = as
            GRADSLAM_HIP_DETERMINISTIC_BACKWARD says when the backward runs.
        pixel_weights: None (the default: no weights, the solves above bit for bit) or a callable that takes the live
            `RGBDImages` the solve sees and returns the per-pixel weights of its frames as a float32 tensor (B, H, W) or
            (B, 1, H, W) on the frames' device (`ops.projective_icp_batch(pixel_weights=...)`): a mask, a sensor model
            (`axial_noise_weights`), a network's confidence.  A pixel whose weight is not a positive finite number is
            masked for the solve (the map update still sees it).  It is called once per `localize`.  With
            `differentiable=True` its output stays on the autograd tape: the parameters of a module get gradients.  Works
            with every threshold and with `color_weight`.
        outlier_mask: None (the default: the calls and the pose bits above) or a dict with any of the keys hi, lo, floor,
            min_support, grow, grow_depth (`ops.projective_icp_outliers_batch`; defaults 3.0, 1.5, 0.0, 6, 0, 0.02) and
            refine_iters (default 5).  `localize` then runs the configured solve, builds the outlier mask at the poses it
            reached (they stay on the device), and runs refine_iters more iterations of the same solve from those poses
            with the masked pixels' weights set to 0 (the caller's `pixel_weights` elsewhere, or ones).  The mask of the
            last call is kept in `last_outlier_mask` (B, H, W) bool.  Works with every threshold, `color_weight` and
            `pixel_weights`; with `differentiable=True` the mask is a constant of the gradient like the association, the
            two solves are two taped calls chained through the initial pose, and weights that require grad get their
            gradient through the `torch.where` that applies the mask.  The parameters are starting points, not tuned to
            any sensor.
        surfel_radii: False (the default: the calls and the pose bits above) or True: the model view is rendered with
            the radii of the map's `SurfelRadii` layer (`Pointclouds.render(radii="layer")`), so a view nearer than the
            capture keeps its pairs and a farther one does not fatten its edges.  `radius` must then be 0, and a map
            without the layer raises.  Nothing else of the solve changes (it already accepts a surfel behind several
            pixels): it works with every threshold, `color_weight`, `pixel_weights`, `outlier_mask` and
            `differentiable=True` (the radii are constants of the gradient).
        max_radius: 0..8, the cap of a surfel's square in pixels with `surfel_radii`

    Unlike the point-cloud-pair providers it needs the map and the live frame themselves: call
    `localize(pointclouds, live_frame, prev_poses)`."""

    def __init__(self, numiters: int = 10, damp: float = 1e-8, dist_thresh: Union[float, int] = 0.1,
                 angle_thresh: Union[float, int] = 30, stride: Optional[int] = None,
                 min_confidence: Union[float, int] = 0.0, radius: int = 0, differentiable: bool = False,
                 color_weight: Union[float, int] = 0.0, huber_delta: Union[float, int] = 0.0,
                 color_huber_delta: Union[float, int] = 0.0, huber_k: Union[float, int] = 0.0,
                 color_huber_k: Union[float, int] = 0.0, deterministic_backward: Optional[bool] = None,
                 pixel_weights: Optional[Callable] = None, outlier_mask: Optional[dict] = None,
                 surfel_radii: bool = False, max_radius: int = 3):
        from .. import ops
        who = "ProjectiveICPOdometryProvider"
        if not isinstance(surfel_radii, bool):
            raise TypeError("surfel_radii must be of type bool; but was of type {}.".format(type(surfel_radii)))
        ops._render_radii(who, (), None, 0, max_radius)
        if surfel_radii and radius != 0:
            raise ValueError("{}: radius ({}) must be 0 with surfel_radii: every surfel brings its own square (cap it "
                             "with max_radius)".format(who, radius))
        self.surfel_radii, self.max_radius = surfel_radii, max_radius
        if pixel_weights is not None and not callable(pixel_weights):
            raise TypeError("pixel_weights must be None or a callable (live frame -> weights); but was of type "
                            "{}.".format(type(pixel_weights)))
        self.pixel_weights = pixel_weights
        if not isinstance(differentiable, bool):
            raise TypeError("differentiable must be of type bool; but was of type {}.".format(type(differentiable)))
        ops._picp_deterministic(who, "deterministic_backward", deterministic_backward)
        opt = ops._picp_options(who, geometry=(1 if stride is None else stride, numiters, damp, dist_thresh, angle_thresh),
                                color_weight=color_weight)
        if color_weight > 0 and differentiable:
            raise ValueError("color_weight > 0 cannot be combined with differentiable=True: the colour term has no "
                             "backward pass yet")
        opt = ops._picp_options(who, opt, huber_delta=huber_delta, color_huber_delta=color_huber_delta)
        if color_huber_delta > 0 and not color_weight > 0:
            raise ValueError("color_huber_delta > 0 needs color_weight > 0: it is the Huber threshold of the colour term")
        opt = ops._picp_options(who, opt, huber_k=huber_k, color_huber_k=color_huber_k)
        if color_huber_k > 0 and not color_weight > 0:
            raise ValueError("color_huber_k > 0 needs color_weight > 0: it estimates the Huber threshold of the colour "
                             "term")
        # (validated after every other keyword: the refusals above and their order stay)
        self.outlier_rule, self.refine_iters = self._outlier_mask(outlier_mask)
        self.outlier_mask = None if outlier_mask is None else dict(outlier_mask)
        self.last_outlier_mask = None
        # What every solve of localize runs with, fixed here: the validated record.  The attributes below are the values
        # as they were given, for the SLAM drivers and callers to read (the first five make _kwargs()); assigning to
        # one of them after construction does NOT reach localize -- build a new provider instead.
        self.options = opt._replace(deterministic=deterministic_backward)
        self.numiters = numiters
        self.damp = damp
        self.dist_thresh = dist_thresh
        self.angle_thresh = angle_thresh
        self.stride = stride
        self.color_weight = color_weight
        self.huber_delta = huber_delta
        self.color_huber_delta = color_huber_delta
        self.huber_k = huber_k
        self.color_huber_k = color_huber_k
        self.deterministic_backward = deterministic_backward
        self.min_confidence = min_confidence
        self.radius = radius
        self.differentiable = differentiable

    @staticmethod
    def _outlier_mask(outlier_mask):
        """(ops.OutlierRule, refine_iters) of the `outlier_mask` keyword, or (None, 0)"""
        from .. import ops
        if outlier_mask is None:
            return None, 0
        if not isinstance(outlier_mask, dict):
            raise TypeError("outlier_mask must be None or a dict (hi, lo, floor, min_support, grow, grow_depth, "
                            "refine_iters); but was of type {}.".format(type(outlier_mask)))
        unknown = sorted(set(outlier_mask) - set(ops.OutlierRule._fields) - {"refine_iters"}, key=str)
        if unknown:
            raise TypeError("outlier_mask: unknown keys {}; it takes {} and refine_iters".format(
                unknown, ", ".join(ops.OutlierRule._fields)))
        rule = ops._outlier_rule("outlier_mask", **{k: v for k, v in outlier_mask.items() if k != "refine_iters"})
        refine_iters = outlier_mask.get("refine_iters", 5)
        if isinstance(refine_iters, bool) or not isinstance(refine_iters, int):
            raise TypeError("outlier_mask: refine_iters must be of type int; but was of type {}.".format(
                type(refine_iters)))
        if refine_iters < 1:
            raise ValueError("outlier_mask: refine_iters ({}) must be at least 1.".format(refine_iters))
        return rule, refine_iters

    def _kwargs(self):
        return dict(stride=1 if self.stride is None else self.stride, numiters=self.numiters, damp=self.damp,
                    dist_thresh=self.dist_thresh, angle_thresh=self.angle_thresh)

    def _weights(self, live_frame, B, H, W):
        """the weight image of a localisation (B, H, W), or None: ONE call of the caller's function"""
        if self.pixel_weights is None:
            return None
        w = self.pixel_weights(live_frame)
        if not torch.is_tensor(w):
            raise TypeError("pixel_weights must return a tensor; got {}.".format(type(w)))
        if tuple(w.shape) not in ((B, H, W), (B, 1, H, W)):
            raise ValueError("pixel_weights must return a tensor of shape {} or {}; got {}.".format(
                (B, H, W), (B, 1, H, W), tuple(w.shape)))
        if w.dtype != torch.float32:
            raise TypeError("pixel_weights must return a float32 tensor; got {}.".format(w.dtype))
        return w.reshape(B, H, W)

    def provide(self, *args, **kwargs):
        raise TypeError("ProjectiveICPOdometryProvider aligns a live frame with the rendered map, not two point clouds: "
                        "call localize(pointclouds, live_frame, prev_poses)")

    def localize(self, pointclouds: Pointclouds, live_frame: RGBDImages, prev_poses: torch.Tensor) -> torch.Tensor:
        r"""Poses (B, 1, 4, 4) of `live_frame` (B sequences, one frame each) against the map `pointclouds`, starting from
        `prev_poses` (B, 1, 4, 4) or (B, 4, 4), at which the model view is rendered.  The map is read in place; counts
        that live on the device stay there."""
        if not isinstance(pointclouds, Pointclouds):
            raise TypeError("Expected pointclouds to be of type gradslam.Pointclouds. Got {0}.".format(type(pointclouds)))
        if not isinstance(live_frame, RGBDImages):
            raise TypeError("Expected live_frame to be of type gradslam.RGBDImages. Got {0}.".format(type(live_frame)))
        if not torch.is_tensor(prev_poses):
            raise TypeError("Expected prev_poses to be of type tensor. Got {0}.".format(type(prev_poses)))
        from .. import ops
        fr = live_frame.to_channels_last()
        B, L, H, W = fr.shape
        if L != 1:
            raise ValueError("Expected live_frame to have sequence length of 1. Got {0}.".format(L))
        if len(pointclouds) != B or pointclouds._buf["points"] is None or pointclouds._buf["normals"] is None:
            raise ValueError("Expected a map with points and normals for each of the {0} sequences of live_frame "
                             "(got {1}).".format(B, len(pointclouds)))
        if tuple(prev_poses.shape) not in ((B, 1, 4, 4), (B, 4, 4)):
            raise ValueError("prev_poses should have shape {0}, but had shape {1}".format((B, 1, 4, 4),
                                                                                         tuple(prev_poses.shape)))
        poses = prev_poses.reshape(B, 4, 4).contiguous().float()
        K = fr.intrinsics[:, 0].contiguous().float()
        maps = pointclouds._map_rows(("points", "normals") + (("features",) if self.min_confidence > 0 else ()))
        weights = self._weights(live_frame, B, H, W)
        # The model view, rendered once.  The index image is all the geometric solve reads of it: no colour, normal or
        # confidence image is rendered.  The joint solve reads the view's colour image too.  On the tape the render stays
        # off it (the winners are constants): it sees detached tensors and does not warn
        colour, taped = self.options.color_weight > 0, self.differentiable
        view_maps, view_poses, guard = [m._replace(normals=None) for m in maps], poses, None
        if colour:
            colors = pointclouds._buf["colors"]
            if colors is None or any(c is None for c in colors):
                raise ValueError("color_weight > 0 needs a map with colours")
            view_maps = [m._replace(colors=colors[b]) for b, m in enumerate(view_maps)]
        elif taped:
            view_maps, view_poses = [m._replace(points=m.points.detach()) for m in view_maps], poses.detach()
            key = pointclouds._rewrites()

            def guard():
                if pointclouds._rewrites() != key:
                    raise RuntimeError("the map was changed in place after localize(differentiable=True) and before its "
                                       "backward pass: the saved association no longer belongs to the map rows (run "
                                       "backward before the next in-place PointFusion.step or prune_, or keep the map "
                                       "update on the autograd tape)")
        splat = {}
        if self.surfel_radii:
            from ..structures.mapfeatures import SurfelRadii
            layer = pointclouds.map_features
            if not isinstance(layer, SurfelRadii) or layer._emb is None:
                raise ValueError("surfel_radii needs a SurfelRadii layer on the map (attach_features(SurfelRadii()), or "
                                 "PointFusion(surfel_radii=True))")
            splat = dict(radii=[layer._emb[b][:min(m.n_bound, int(m.points.shape[0])), 0] for b, m in enumerate(maps)],
                         max_radius=self.max_radius)
        view = ops.render_map_batch(view_maps, view_poses.view(B, 1, 4, 4), K, H, W, radius=self.radius,
                                    min_confidence=self.min_confidence, **splat)
        # the joint solve: the view's intensity image and the live colour next to the geometric solve's inputs
        color, model = (fr.rgb_image[:, 0], ops.model_intensity(view.color[:, 0], view.index[:, 0])) if colour \
            else (None, None)
        args = (fr.vertex_map[:, 0], fr.normal_map[:, 0], fr.depth_image[:, 0, ..., 0], K, view.index[:, 0], view_poses,
                maps, poses)
        entries = ops._picp_pixel_weights("projective_icp_color" if colour else "projective_icp", weights, args[2])
        if self.outlier_rule is None:
            if taped:
                return ops._picp_taped(self.options, *args, weights, entries, guard=guard).unsqueeze(1)
            out = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=poses.device)
            ops._picp_solve(self.options, *args, color=color, model=model, out=out.view(B, 4, 4), weights=entries)
            return out
        # The configured solve, the outlier mask at the poses it reached, then refine_iters more iterations of the same
        # solve from those poses without the masked pixels.  Nothing is read back between the three.
        who = "projective_icp_color" if colour else "projective_icp"

        def solve(opt, init, w, w_entries):
            if taped:
                return ops._picp_taped(opt, *args[:7], init, w, w_entries, guard=guard)
            return ops._picp_solve(opt, *args[:7], init, color=color, model=model, weights=w_entries)
        first = solve(self.options, poses, weights, entries)
        with torch.no_grad():   # (a constant of the gradient, like the association)
            mask = ops.projective_icp_outliers_batch(*args[:7], first, dist_thresh=self.dist_thresh,
                                                     angle_thresh=self.angle_thresh, pixel_weights=entries,
                                                     **self.outlier_rule._asdict()).bool()
        base = torch.ones((B, H, W), dtype=torch.float32, device=mask.device) if weights is None else weights
        masked = torch.where(mask, torch.zeros((), dtype=torch.float32, device=mask.device), base)
        self.last_outlier_mask = mask
        return solve(self.options._replace(numiters=self.refine_iters), first, masked,
                     ops._picp_pixel_weights(who, masked, args[2])).unsqueeze(1)
