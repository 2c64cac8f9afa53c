"""A C-channel feature per surfel, kept row-aligned with a `Pointclouds` map (not part of the reference API).

    layer = MapFeatures(512, dtype=torch.float16)
    pointclouds.attach_features(layer)
    slam.step(pointclouds, live, prev, inplace=True, features=clip_image)   # (B, H, W, 512)
    score = layer.similarity(text_embedding)                                # per sequence (N_b,)

The fusion is `ops.fuse_features_batch` (HIP): the weights and the correspondences of the colour fusion.  The layer
follows the map through `prune_`, `carve_`, `voxel_downsample_` and the drivers' schedules
(`ops.compact_features_batch` with the mask the map itself is compacted with)."""
import torch

__all__ = ["MapFeatures", "SurfelRadii"]

_DTYPES = (torch.float32, torch.float16)


class MapFeatures(object):
    r"""Per-sequence capacity-backed feature buffers of one map: `emb` (capacity, C) and `weight` (capacity,).

    Args:
        channels: C, 1 .. 4096
        dtype: torch.float32 or torch.float16 (the arithmetic is float32 either way; a float16 layer is stored rounded
            to nearest even)

    A layer belongs to one map object (`Pointclouds.attach_features`).  `clone()`, indexing and the out-of-place
    `prune` / `carve` / `voxel_downsample` of the map return maps without it."""

    def __init__(self, channels: int, dtype: torch.dtype = torch.float32):
        if not isinstance(channels, int) or isinstance(channels, bool):
            raise TypeError("channels must be of type int; but was of type {}.".format(type(channels)))
        if not 1 <= channels <= 4096:
            raise ValueError("channels ({}) must be in 1..4096.".format(channels))
        if dtype not in _DTYPES:
            raise ValueError("dtype must be torch.float32 or torch.float16; got {}.".format(dtype))
        self.channels, self.dtype = channels, dtype
        self._emb = None      # per sequence (capacity, C)
        self._weight = None   # per sequence (capacity,)
        self._map = None      # the Pointclouds it is attached to
        self.last_row_of_pix = None   # (B, H * W) int32 of the last fused frame: the layer / map row of each pixel, -1 none

    # ------------------------------------------------------------------ buffers
    def _alloc(self, b, cap, keep_rows, device):
        """buffers of sequence b with at least `cap` rows; the first keep_rows rows are carried over"""
        emb = torch.empty((cap, self.channels), dtype=self.dtype, device=device)
        weight = torch.empty((cap,), dtype=torch.float32, device=device)
        if keep_rows:
            emb[:keep_rows] = self._emb[b][:keep_rows]
            weight[:keep_rows] = self._weight[b][:keep_rows]
        self._emb[b], self._weight[b] = emb, weight

    def _bind(self, pointclouds):
        """buffers for the sequences of a map that had none when the layer was attached (an empty map's first step);
        rows the map already holds read zeros with weight 0"""
        B = len(pointclouds._n_host)
        if self._emb is not None and len(self._emb) == B:
            return
        self._emb, self._weight = [None] * B, [None] * B
        for b in range(B):
            bound = pointclouds._count_of(b)[0]
            pts = pointclouds._buf["points"]
            cap = max(bound, int(pts[b].shape[0]) if pts is not None else 0, 1)
            self._alloc(b, cap, 0, pointclouds.device)
            self._emb[b][:bound].zero_()
            self._weight[b][:bound].zero_()

    def _reserve(self, b, bound, extra):
        """room for `extra` more rows behind the first `bound` (geometric growth, as Pointclouds._reserve)"""
        cap = int(self._emb[b].shape[0])
        if bound + extra > cap:
            self._alloc(b, max(bound + extra, 2 * cap, 1024), min(bound, cap), self._emb[b].device)

    # ------------------------------------------------------------------ views
    def _counts(self):
        if self._map is None:
            raise ValueError("the feature layer is not attached to a map")
        return self._map._n

    @property
    def features_list(self):
        """per sequence the (N_b, C) features of the map's rows: views of the live buffers"""
        n = self._counts()
        return [] if self._emb is None else [t[:k] for t, k in zip(self._emb, n)]

    @property
    def weights_list(self):
        """per sequence the (N_b,) fusion weights: the sum of the sample confidences of the valid pixels fused into a row"""
        n = self._counts()
        return [] if self._weight is None else [t[:k] for t, k in zip(self._weight, n)]

    def similarity(self, query: torch.Tensor):
        r"""Cosine similarity of every surfel's feature against `query` ((C,) or (Q, C)): per sequence an (N_b,) or
        (N_b, Q) float32 tensor; a row of weight 0 (no valid pixel ever reached it) scores 0.  Plain torch."""
        if not torch.is_tensor(query) or query.ndim not in (1, 2) or query.shape[-1] != self.channels:
            raise ValueError("query must be a tensor of shape (C,) or (Q, C) with C = {}; got {}".format(
                self.channels, tuple(query.shape) if torch.is_tensor(query) else type(query)))
        out = []
        for f, w in zip(self.features_list, self.weights_list):
            q = query.to(device=f.device, dtype=torch.float32)
            q2 = q if q.ndim == 2 else q.unsqueeze(0)
            s = torch.nn.functional.normalize(f.to(torch.float32), dim=-1) @ torch.nn.functional.normalize(q2, dim=-1).T
            s = torch.where((w > 0).unsqueeze(-1), s, torch.zeros_like(s))
            out.append(s if q.ndim == 2 else s[:, 0])
        return out

    def gather(self, index_image: torch.Tensor):
        r"""Feature images from the index image of `Pointclouds.render(..., return_extras=True)` ((B, L, H, W) int64, the
        map row behind each pixel, negative in holes): (B, L, H, W, C) of the layer's dtype, zeros in holes.  Plain
        torch."""
        n = self._counts()
        if not torch.is_tensor(index_image) or index_image.dtype.is_floating_point or index_image.ndim != 4 or \
                index_image.shape[0] != len(n):
            raise ValueError("index_image must be an integer tensor of shape (B, L, H, W) with B = {}".format(len(n)))
        out = torch.zeros(tuple(index_image.shape) + (self.channels,), dtype=self.dtype, device=index_image.device)
        for b, f in enumerate(self.features_list):
            idx = index_image[b].to(torch.int64)
            hit = (idx >= 0) & (idx < f.shape[0])
            out[b][hit] = f[idx[hit]]
        return out

    # ------------------------------------------------------------------ the passes
    def _frame_features(self, features, features_valid, B, H, W):
        """the checked (B, H, W, C) feature image and (B, H * W) mask of a step, or None each"""
        feat, valid = None, None
        if features is not None:
            if not torch.is_tensor(features):
                raise TypeError("features must be of type tensor; got {}.".format(type(features)))
            if features.ndim == 5 and features.shape[1] == 1:
                features = features[:, 0]
            if tuple(features.shape) != (B, H, W, self.channels):
                raise ValueError("features must have shape {} or {}; got {}".format(
                    (B, 1, H, W, self.channels), (B, H, W, self.channels), tuple(features.shape)))
            if features.dtype != self.dtype:
                raise ValueError("features must have the layer's dtype {}; got {}".format(self.dtype, features.dtype))
            feat = features
        if features_valid is not None:
            if features is None:
                raise ValueError("features_valid was given without features")
            if not torch.is_tensor(features_valid) or features_valid.dtype not in (torch.bool, torch.uint8):
                raise TypeError("features_valid must be a bool / uint8 tensor")
            if features_valid.ndim == 4 and features_valid.shape[1] == 1:
                features_valid = features_valid[:, 0]
            if tuple(features_valid.shape) != (B, H, W):
                raise ValueError("features_valid must have shape {} or {}; got {}".format(
                    (B, 1, H, W), (B, H, W), tuple(features_valid.shape)))
            valid = features_valid
        return feat, valid

    def _fuse(self, pointclouds, record, depth, alpha, feat, valid):
        """the pass of one step, after the map update that left `record` (best_pix, the old counts) behind"""
        from .. import ops
        self._bind(pointclouds)
        B, H, W = depth.shape
        best, n_old = record
        if isinstance(best, (list, tuple)):
            best = torch.stack([t.reshape(-1) for t in best])
        for b in range(B):
            self._reserve(b, int(n_old[b][0]), H * W)
        r = ops.fuse_features_batch(list(zip(self._emb, self._weight)), n_old, best, depth, alpha, feat, valid)
        self.last_row_of_pix = r.row_of_pix
        return r

    def _compact(self, n, keeps):
        """follows a prune of the map: the same rows, by the same mask (HIP)"""
        from .. import ops
        r = ops.compact_features_batch(list(zip(self._emb, self._weight)), n, keeps)
        for b, (emb, weight) in enumerate(r.layers):
            self._emb[b], self._weight[b] = emb, weight
        return r.counts

    def _select(self, b, rows, selection):
        """follows a prune of the map through boolean indexing (CPU maps, maps on the autograd tape)"""
        self._emb[b] = self._emb[b][:rows][selection]
        self._weight[b] = self._weight[b][:rows][selection]


class SurfelRadii(MapFeatures):
    r"""The radius of every surfel (Keller et al.), as a one-channel float32 layer that makes its own feature image:

        pointclouds.attach_features(SurfelRadii())
        slam.step(pointclouds, live, prev, inplace=True)                 # no features=: the layer samples the frame
        view = pointclouds.render(K, poses, H, W, radii="layer")

    On every in-place `PointFusion.step` the frame the map update saw yields a radius per pixel (`ops.surfel_radius` on
    its depth, local normal map and intrinsics: 0.7071 z / f over |n_z|, at most twice the fronto-parallel value), which
    is fused like any feature with the colours' weights: a matched surfel takes the confidence-weighted mean, an appended
    one its sample's radius; a pixel without a usable normal leaves a matched surfel alone and appends radius 0, weight 0.
    `features=` on such a map raises.  `radii_list` are the (N_b,) radii in metres."""

    def __init__(self):
        super().__init__(1, torch.float32)

    @property
    def radii_list(self):
        """per sequence the (N_b,) radii of the map's rows: views of the live buffers"""
        return [f[:, 0] for f in self.features_list]

    def _frame_features(self, features, features_valid, B, H, W):
        if features is not None or features_valid is not None:
            raise ValueError("features were given, but the map's layer is a SurfelRadii: it makes its own feature image "
                             "from the frame (a map has one layer; pass radii= to render explicitly to keep yours)")
        return None, None

    def _sample(self, frame):
        """(feat (B, H, W, 1), valid (B, H, W)) of a channels-last frame of sequence length 1"""
        from .. import ops
        radius, valid = ops.surfel_radius(frame.depth_image[:, 0, ..., 0].detach(), frame.normal_map[:, 0].detach(),
                                          frame.intrinsics[:, 0].detach())
        return radius.unsqueeze(-1), valid
