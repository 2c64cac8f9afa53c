"""gradslam_amd — MI355X-native dense-SLAM hot path behind gradslam's Python API.

    from gradslam_amd import RGBDImages, Pointclouds
    from gradslam_amd.slam import PointFusion, ICPSLAM

Same classes, functions, argument meaning and error behaviour as gradslam v0.1.0 for the path
depth -> vertex/normal maps -> (grad)ICP odometry -> PointFusion map update; the bodies are
hand-written HIP kernels for gfx950 in gradslam_amd/csrc (C-ABI: include/gradslam_hip.h).
The HIP library is loaded on first use and there is no CPU / PyTorch fallback.

Beyond the reference: `Pointclouds.render` (the model view: the map seen from camera poses, optionally differentiable)
and `Pointclouds.mark_epoch / prune_ / prune` with `PointFusion(prune_min_confidence=..., prune_min_age=...,
prune_every=...)` (off by default): a stable, batched compaction of the map that removes surfels whose confidence stays
below a threshold after a number of steps, without a read-back and without a per-surfel age channel;
`RGBDImages.bilateral_filter` with `ICPSLAM / PointFusion(depth_filter=...)` (off by default): the edge-preserving
pre-pass on the raw depth in front of the vertex and normal maps, differentiable down to the sensor depth;
`MapFeatures` with `Pointclouds.attach_features` and `PointFusion.step(..., features=...)` (off by default): a C-channel
feature per surfel, fused from per-pixel feature images with the weights and the correspondences of the colour fusion
and kept row-aligned with the map through pruning, carving and thinning."""
from .version import __version__  # noqa: F401
from .geometry import *  # noqa: F401,F403
from . import odometry, slam, metrics  # noqa: F401
from .structures import *  # noqa: F401,F403
