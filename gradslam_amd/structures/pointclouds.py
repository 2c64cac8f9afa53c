"""Batched variable-length pointcloud / surfel map with the interface of the reference's
`gradslam.Pointclouds` (structures/pointclouds.py:13-1467), re-designed around growth:

  * every sequence b owns CAPACITY-BACKED buffers points/normals/colors (cap, 3) and features
    (cap, F); the HIP fuse/append kernels write new surfels in place and only the count
    changes.  Capacity grows geometrically, so a 500-frame sequence reallocates O(log N) times
    instead of re-concatenating and re-padding every attribute every frame
    (reference: pointclouds.py:1203-1228, :948-995);
  * `*_list` are zero-copy views buf[:n]; `*_padded` is a zero-copy view when the batch has
    one sequence (the one-sequence-per-GPU layout) and is materialised lazily otherwise.

Only the container logic lives here (torch as memory plumbing); the arithmetic of the SLAM path
is in libgradslam_hip.so.
"""
import time
from typing import List, Optional, Union

import torch

__all__ = ["Pointclouds"]

_ATTRS = ("points", "normals", "colors", "features")


def _canon_device(device):
    return torch.Tensor().to(device).device


def _voxel_keep_torch(points, confidence, voxel_size):
    """The rule of gs_voxel.hip in torch, for maps the kernel does not serve (CPU maps): points (n, 3), confidence (n,) or
    None, voxel_size a float that float32 holds.  Voxel q_c = floor(p_c / voxel_size) in float32; griddable iff p is
    finite and -2^20 <= q_c < 2^20; score = the bit pattern of the confidence when >= +0.0 (else 0; -0.0 as +0.0); per
    voxel the largest score wins, the lowest row among equals.  Returns (keep uint8 (n,), winner int64 (n,))."""
    n = int(points.shape[0])
    dev = points.device
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.zeros(0, dtype=torch.uint8, device=dev), rows
    p = points.to(torch.float32)
    q = torch.floor(p / torch.tensor(voxel_size, dtype=torch.float32, device=dev))
    grid = (torch.isfinite(p) & (q >= -1048576.0) & (q < 1048576.0)).all(dim=1)
    qi = torch.where(grid.unsqueeze(1), q, torch.zeros_like(q)).to(torch.int64) + (1 << 20)
    key = (qi[:, 0] << 42) | (qi[:, 1] << 21) | qi[:, 2]
    if confidence is None:
        score = torch.zeros(n, dtype=torch.int64, device=dev)
    else:
        c = confidence.to(torch.float32).contiguous()
        score = torch.where(c >= 0, c.view(torch.int32).to(torch.int64) & 0x7FFFFFFF, torch.zeros((), dtype=torch.int64,
                                                                                                  device=dev))
    winner = rows.clone()
    g = torch.nonzero(grid).reshape(-1)
    if g.numel():
        _, inv = torch.unique(key[g], return_inverse=True)
        word = (score[g] << 32) | (0xFFFFFFFF - g)          # larger: the larger score, then the lower row
        best = torch.zeros(int(inv.max()) + 1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, word, "amax")
        winner[g] = 0xFFFFFFFF - (best[inv] & 0xFFFFFFFF)
    return (winner == rows).to(torch.uint8), winner


class _CountGroup(object):
    """Surfel counts of the sequences of a batch that live ON THE DEVICE (written by the fuse/append kernels).

    The host only keeps upper bounds (launch geometry, capacity).  Every EVERY-th update queues ONE asynchronous
    copy of all the counts into pinned memory; `poll()` tightens the bounds from the copies that have already landed
    and never waits, so the frame loop has no host<->device sync."""
    RING = 8
    wait_s = 0.0    # seconds the host has spent waiting in `advance` (class-wide; bench.py reports host time without it)
    EVERY = 2       # one asynchronous read-back per EVERY updates (a copy + an event on the stream)
    MAX_AHEAD = 2   # read-backs in flight before the host waits for the oldest: the host never runs more than
                    # ~EVERY * (MAX_AHEAD + 1) frames ahead of the device, which keeps the bounds (launch sizes,
                    # capacity) within a few frames of the true counts while the device always has work queued

    def __init__(self, dev, bounds):
        self.dev, self.bounds = dev, [int(x) for x in bounds]   # dev: (B,) int64 on the device
        self._updates = 0
        self._pin = torch.empty((self.RING, len(self.bounds)), dtype=torch.int64).pin_memory()
        self._events = [torch.cuda.Event() for _ in range(self.RING)]
        self._pending = []   # [slot, rows that may have been added to every sequence since that copy]
        self._slot = 0
        self._queue_copy()

    def _queue_copy(self):
        if len(self._pending) == self.RING:
            return
        s = self._slot
        self._slot = (s + 1) % self.RING
        self._pin[s].copy_(self.dev, non_blocking=True)
        self._events[s].record()
        self._pending.append([s, 0])

    def advance(self, dev, max_growth):
        g = int(max_growth)
        self.dev = dev
        self.bounds = [x + g for x in self.bounds]
        for p in self._pending:
            p[1] += g
        self._updates += 1
        if self._updates % self.EVERY == 0:
            self._queue_copy()
            if len(self._pending) > self.MAX_AHEAD:
                t0 = time.perf_counter()
                self._events[self._pending[0][0]].synchronize()   # frames old: the device is still busy behind it
                _CountGroup.wait_s += time.perf_counter() - t0
        self.poll()

    def shrink(self, dev):
        """A prune wrote smaller counts to `dev`.  The host bounds stay as they are: they, and the read-backs already in
        flight (counts from before the prune), remain upper bounds.  One more read-back is queued, so that `poll()`
        tightens the bounds to the pruned counts without a wait."""
        self.dev = dev
        self._queue_copy()

    def poll(self):
        while self._pending and self._events[self._pending[0][0]].query():
            s, grown = self._pending.pop(0)
            self.bounds = [min(x, v + grown) for x, v in zip(self.bounds, self._pin[s].tolist())]

    def resolve(self):
        return [int(v) for v in self.dev.cpu().tolist()]

    def tighten(self):
        """One sync: the bounds become the exact counts (used before a buffer would be reallocated: the bounds run a
        few frames x H*W rows ahead of the counts, which for a 1296x968 frame is millions of rows)."""
        vals = self.resolve()
        self.poll()          # every queued copy has landed by now
        self.bounds = vals
        return vals


class _DeviceCount(object):
    """The count of ONE sequence inside a _CountGroup (the group does the read-backs for all its sequences)."""

    def __init__(self, group, index):
        self.group, self.index = group, index

    @property
    def bound(self):
        return self.group.bounds[self.index]

    @property
    def dev(self):
        return self.group.dev[self.index:self.index + 1]

    def poll(self):
        self.group.poll()

    def resolve(self):
        return int(self.dev.item())


class Pointclouds(object):
    r"""Batch of pointclouds (with varying numbers of points).

    Args:
        points (list of (N_b, 3) tensors, or (B, N, 3) tensor, or None)
        normals, colors: same container type and shapes as `points`, or None
        features: list of (N_b, F) tensors or (B, N, F) tensor, or None
        device: device of the internal tensors (default: that of `points`, or cpu when empty)
    """

    def __init__(
        self,
        points: Union[List[torch.Tensor], torch.Tensor, None] = None,
        normals: Union[List[torch.Tensor], torch.Tensor, None] = None,
        colors: Union[List[torch.Tensor], torch.Tensor, None] = None,
        features: Union[List[torch.Tensor], torch.Tensor, None] = None,
        device: Union[torch.device, str, None] = None,
    ):
        if not (points is None or isinstance(points, list) or torch.is_tensor(points)):
            raise TypeError("Expected points to be of type list or tensor or None; got %r" % type(points))
        for name, val in (("normals", normals), ("colors", colors), ("features", features)):
            if not (val is None or isinstance(val, type(points))):
                raise TypeError("Expected %s to be of same type as points (%r); got %r"
                                % (name, type(points), type(val)))
        if points is not None and len(points) == 0:
            raise ValueError("len(points) (= 0) should be > 0")

        self._buf = {k: None for k in _ATTRS}   # per attribute: list of (cap_b, C) tensors or None
        self._dcount = {}                       # b -> _DeviceCount while the count of b is device-side
        self._n_host: List[int] = []            # points per sequence (see the `_n` property)
        self._padded_cache = {}
        self._generation = 0   # bumped by everything that changes the map in place (see render(differentiable=True))
        self._taped_swaps = 0  # of those, the ones that leave the old buffers as they were: taped map updates (new
        #                        autograd tensors) and read-backs of the device counts (_rewrites)
        self._marks = None      # (B, MAX_MARKS) int64 on self.device: the counts at the last _n_marks epochs (mark_epoch)
        self._n_marks = 0
        self._prune_steps = 0   # steps a pruning PointFusion has taken on this map (the step counter lives with the map)
        self._carve_steps = 0   # the same for a carving PointFusion (carve_margin)
        self._voxel_steps = 0   # the same for a thinning PointFusion (voxel_size)
        self.last_pruned = None  # (B,) int64: rows the last prune_ removed per sequence (on the map's device, never synced)
        self._feature_layer = None   # the MapFeatures attached to this object (attach_features); copies come without it
        self._fuse_record = None     # with a layer: (best_pix, [(old bound, old device count)]) of the last map update
        self.equisized = None

        if isinstance(points, list):
            shapes = [p.shape for p in points]
            if any(p.ndim != 2 for p in points):
                raise ValueError("ndim of all tensors in points list should be 2")
            if any(s[-1] != 3 for s in shapes):
                raise ValueError("last dim of all tensors in points should have shape 3 (X, Y, Z)")
            self.device = _canon_device(device) if device is not None else points[0].device
            if not (normals is None or [n.shape for n in normals] == shapes):
                raise ValueError("normals tensors should have same shape as points tensors, but didn't")
            if not (colors is None or [c.shape for c in colors] == shapes):
                raise ValueError("colors tensors should have same shape as points tensors, but didn't")
            if not (features is None or all(f.ndim == 2 for f in features)):
                raise ValueError("ndim of all tensors in features list should be 2")
            if not (features is None or [len(f) for f in features] == [s[0] for s in shapes]):
                raise ValueError("number of features per pointcloud has to be equal to number of points")
            if not (features is None or len(set(f.shape[-1] for f in features)) == 1):
                raise ValueError("number of features per pointcloud has to be the same")
            self._n = [int(s[0]) for s in shapes]
            for k, val in zip(_ATTRS, (points, normals, colors, features)):
                self._buf[k] = None if val is None else [v.to(self.device) for v in val]
            self.equisized = len(set(self._n)) == 1
        elif torch.is_tensor(points):
            self.device = _canon_device(device) if device is not None else points.device
            if points.ndim != 3:
                raise ValueError("points should have ndim=3, but had ndim={}".format(points.ndim))
            if points.shape[-1] != 3:
                raise ValueError("last dim of points should have shape 3 (X, Y, Z) but had shape %r"
                                 % (points.shape[-1]))
            if points.shape[0] == 0:
                raise ValueError("Batch size of 0 not supported yet. Got input points shape {}.".format(points.shape))
            if not (normals is None or normals.shape == points.shape):
                raise ValueError("normals tensor should have same shape as points tensor, but didn't: %r != %r"
                                 % (normals.shape, points.shape))
            if not (colors is None or colors.shape == points.shape):
                raise ValueError("colors tensor should have same shape as points tensor, but didn't: %r != %r"
                                 % (colors.shape, points.shape))
            if not (features is None or features.ndim == 3):
                raise ValueError("features should have ndim=3, but had ndim={}".format(features.ndim))
            if not (features is None or features.shape[:-1] == points.shape[:-1]):
                raise ValueError("first 2 dims of features tensor and points tensor should have same shape, "
                                 "but didn't: %r != %r" % (features.shape[:-1], points.shape[:-1]))
            B, N = points.shape[:2]
            self._n = [int(N)] * B
            for k, val in zip(_ATTRS, (points, normals, colors, features)):
                self._buf[k] = None if val is None else [val[b].to(self.device) for b in range(B)]
            self.equisized = True
        else:
            self.device = _canon_device(device) if device is not None else torch.device("cpu")

    # ------------------------------------------------------------------ basic protocol
    @property
    def _n(self):
        """Points per sequence.  Reading it resolves device-side counts (one read-back each)."""
        if self._dcount:
            exact = {}   # one read-back per group
            for b, dc in self._dcount.items():
                if id(dc.group) not in exact:
                    exact[id(dc.group)] = dc.group.resolve()
                self._n_host[b] = exact[id(dc.group)][dc.index]
            self._dcount = {}
            self._invalidate()
            self._taped_swaps += 1   # (a count read back: the buffers hold what they held, see _rewrites)
        return self._n_host

    @_n.setter
    def _n(self, value):
        self._n_host = value
        self._dcount = {}

    def __len__(self):
        return len(self._n_host)

    @property
    def _B(self):
        return len(self._n_host)

    @property
    def _N(self):
        return max(self._n) if self._n else 0

    def __getitem__(self, index):
        if not self.has_points:
            raise IndexError("cannot index an empty Pointclouds")
        if isinstance(index, int):
            ids = [index]
        elif isinstance(index, slice):
            ids = list(range(len(self)))[index]
        elif isinstance(index, list):
            ids = index
        elif torch.is_tensor(index):
            if index.dim() != 1 or index.dtype.is_floating_point:
                raise IndexError(index)
            ids = index.nonzero().flatten().tolist() if index.dtype == torch.bool else index.tolist()
        else:
            raise IndexError(index)
        if len(ids) == 0:
            raise IndexError("Incorrect indexing at dimension 0, make sure range is within 0 and %d" % len(self))
        lists = {k: (None if self._buf[k] is None else [self._buf[k][i][: self._n[i]] for i in ids]) for k in _ATTRS}
        other = Pointclouds(lists["points"], lists["normals"], lists["colors"], lists["features"])
        other._carry_epochs(self, ids)
        return other

    # ------------------------------------------------------------------ has_*
    @property
    def has_points(self):
        return self._buf["points"] is not None and any(n > 0 for n in self._n)

    @property
    def has_normals(self):
        return self._buf["normals"] is not None

    @property
    def has_colors(self):
        return self._buf["colors"] is not None

    @property
    def has_features(self):
        return self._buf["features"] is not None

    @property
    def num_features(self):
        return None if not self.has_features else self._buf["features"][0].shape[-1]

    @property
    def num_points_per_pointcloud(self):
        return torch.tensor(self._n if self._n else [0], device=self.device)

    # ------------------------------------------------------------------ list / padded views
    def _list(self, k):
        if self._buf[k] is None:
            return None
        return [t[:n] for t, n in zip(self._buf[k], self._n)]

    def _padded(self, k):
        if self._buf[k] is None:
            return None
        if len(self._n) == 1:  # zero-copy: the one-sequence-per-GPU layout
            return self._buf[k][0][: self._n[0]].unsqueeze(0)
        key = (k, tuple(self._n))
        hit = self._padded_cache.get(k)
        if hit is not None and hit[0] == key:
            return hit[1]
        N, C = self._N, self._buf[k][0].shape[-1]
        out = torch.zeros((len(self._n), N, C), dtype=self._buf[k][0].dtype, device=self.device)
        for b, (t, n) in enumerate(zip(self._buf[k], self._n)):
            out[b, :n] = t[:n]
        self._padded_cache[k] = (key, out)
        return out

    # list representation: zero-copy views; the setters follow the reference (structures/pointclouds.py:824-878,
    # :1431-1467: same container type, length and per-sequence shapes, values are cloned)
    def _set_list(self, k, value, first_dim_only=False):
        self._refuse_with_features("setting " + k)
        if not isinstance(value, list):
            raise TypeError("value must be list of torch.Tensors. Got {}".format(type(value)))
        if not self.has_points:
            raise ValueError("cannot set list representation for an empty pointclouds object")
        if len(self) != len(value):
            raise ValueError("value must have same length as pointclouds.points_list. Got {} != {}.".format(
                len(value), len(self)))
        if any(v.ndim != 2 for v in value):
            raise ValueError("ndim of all tensors in value list should be 2")
        pts = self.points_list
        if first_dim_only and any(pts[b].shape[:1] != value[b].shape[:1] for b in range(len(self))):
            raise ValueError("shape of first 2 dims of tensors in value and pointclouds.points_list must match")
        if (not first_dim_only) and any(pts[b].shape != value[b].shape for b in range(len(self))):
            raise ValueError("shape of tensors in value and pointclouds.points_list must match")
        self._store_rows(k, [v.to(self.device) for v in value])

    def _store_rows(self, k, rows):
        """New values of attribute k (one (n_b, C) tensor per sequence) on buffers that keep the CAPACITY of the
        sequence's points buffer: the in-place kernels size every attribute by that capacity (an exact-size clone here
        would be overrun by the next fuse / append)."""
        out = []
        for b, v in enumerate(rows):
            n = int(v.shape[0])
            ref = self._buf["points"][b] if self._buf["points"] is not None else None
            cap = max(n, int(ref.shape[0]) if ref is not None else n)
            buf = torch.empty((cap, v.shape[-1]), dtype=v.dtype, device=self.device)
            buf[:n] = v
            out.append(buf)
        self._buf[k] = out
        self._padded_cache.pop(k, None)

    points_list = property(lambda self: self._list("points"), lambda self, v: self._set_list("points", v))
    normals_list = property(lambda self: self._list("normals"), lambda self, v: self._set_list("normals", v))
    colors_list = property(lambda self: self._list("colors"), lambda self, v: self._set_list("colors", v))
    features_list = property(lambda self: self._list("features"), lambda self, v: self._set_list("features", v, True))

    @property
    def points_padded(self):
        return self._padded("points")

    @property
    def normals_padded(self):
        return self._padded("normals")

    @property
    def colors_padded(self):
        return self._padded("colors")

    @property
    def features_padded(self):
        return self._padded("features")

    @property
    def nonpad_mask(self):
        if not self._n:
            return None
        ar = torch.arange(self._N, device=self.device).unsqueeze(0)
        return ar < torch.tensor(self._n, device=self.device).unsqueeze(1)

    def _set_padded(self, k, value, channels=None):
        self._refuse_with_features("setting " + k)
        if value is None:
            self._buf[k] = None
            return
        if not torch.is_tensor(value):
            raise TypeError("value must be torch.Tensor. Got {}".format(type(value)))
        if not self._n:
            raise ValueError("cannot set padded representation for an empty pointclouds object")
        C = channels if channels is not None else value.shape[-1]
        if value.ndim != 3 or tuple(value.shape) != (len(self._n), self._N, C):
            raise ValueError("value must have shape {}, but had shape {}".format((len(self._n), self._N, C),
                                                                                 tuple(value.shape)))
        if value.device != self.device:
            raise ValueError("value must have the same device as pointclouds object: {} != {}".format(
                value.device, self.device))
        self._store_rows(k, [value[b, :n] for b, n in enumerate(self._n)])

    @points_padded.setter
    def points_padded(self, value):
        self._set_padded("points", value, 3)

    @normals_padded.setter
    def normals_padded(self, value):
        self._set_padded("normals", value, 3)

    @colors_padded.setter
    def colors_padded(self, value):
        self._set_padded("colors", value, 3)

    @features_padded.setter
    def features_padded(self, value):
        self._set_padded("features", value)

    # ------------------------------------------------------------------ surfel-store interface
    # (used by gradslam_amd.slam.fusionutils; not part of the reference API)
    def _invalidate(self):
        self._generation += 1
        self._padded_cache.clear()
        self.equisized = (len(set(self._n)) == 1) if self._n else None

    def _rewrites(self):
        """How often the buffers were rewritten or exchanged behind autograd's back (in-place steps through raw
        pointers, reallocation, prune_).  A taped map update (_fuse_differentiable / _aggregate_differentiable) hands
        the object new autograd tensors and leaves the old ones -- which a saved backward holds -- as they were, and
        reading `_n` only resolves device-side counts: both count in _generation but not here (the guard of ProjectiveICPOdometryProvider.localize)."""
        return self._generation - self._taped_swaps

    RESERVE_FRAMES = 16   # capacity a SLAM driver asks for up front, in frames (see _reserve)

    def _init_empty_batch(self, B, num_features, with_normals=True, with_colors=True):
        """Turns an empty map into B empty sequences with the given attribute set."""
        assert not self._n
        self._n = [0] * B
        mk = lambda c: [torch.empty((0, c), dtype=torch.float32, device=self.device) for _ in range(B)]  # noqa: E731
        self._buf["points"] = mk(3)
        self._buf["normals"] = mk(3) if with_normals else None
        self._buf["colors"] = mk(3) if with_colors else None
        self._buf["features"] = mk(num_features) if num_features else None

    def _reserve(self, b, extra, frames_ahead=1):
        """Guarantees room for `extra` more rows in sequence b (geometric growth) and returns the
        capacity-backed buffers (points, normals, colors, features).  `frames_ahead`: the SLAM drivers, which
        append up to `extra` rows per frame for many frames, ask for several frames of room at once."""
        n_b = self._count_of(b)[0]
        need = n_b + int(extra)
        # (the smallest buffer counts: every attribute is written up to the same row)
        cap = min(self._buf[k][b].shape[0] for k in _ATTRS if self._buf[k] is not None)
        if need > cap and b in self._dcount:
            # the host only knows an upper bound of the count: one sync for the exact value is cheaper than copying the
            # map into buffers twice the size (and re-sizing every scratch that follows the capacity) frames early --
            # unless the bound would be back at the capacity within the few frames the host runs ahead (then every one
            # of those frames would sync here): grow now
            grp = self._dcount[b].group
            grp.tighten()
            n_b = self._count_of(b)[0]
            ahead = grp.EVERY * (grp.MAX_AHEAD + 1) + 2
            need = n_b + int(extra) * (ahead if frames_ahead > 1 else 1)
        if need > cap:
            # geometric growth, starting at RESERVE_FRAMES x the request: a surfel map of a few hundred MB is
            # nothing in 288 GB of HBM, and every reallocation (and every size class the bound-sized per-frame
            # temporaries move through) is a hipMalloc in the middle of a sequence
            new_cap = max(need, int(cap * 2), int(frames_ahead) * int(extra), 1024)
            for k in _ATTRS:
                if self._buf[k] is None:
                    continue
                old = self._buf[k][b]
                if old.shape[0] >= new_cap:
                    continue
                new = torch.empty((new_cap, old.shape[-1]), dtype=old.dtype, device=self.device)
                new[:n_b] = old[:n_b]
                self._buf[k][b] = new
            self._generation += 1
            self._padded_cache.clear()
        return tuple(None if self._buf[k] is None else self._buf[k][b] for k in _ATTRS)

    def _set_count(self, b, n):
        self._n[b] = int(n)
        self._invalidate()

    def _count_of(self, b):
        """(upper bound on the host, device int64[1] tensor or None when the host count is exact)."""
        dc = self._dcount.get(b)
        if dc is None:
            return self._n_host[b], None
        dc.poll()
        return dc.bound, dc.dev

    def _map_rows(self, attrs=_ATTRS):
        """The `maps` argument of the batched map passes of ops: one ops.MapRows per sequence over the buffers, read in
        place; attributes not in `attrs`, or absent, are None.  The counts come from _count_of: a device-side count is
        never forced to the host."""
        from .. import ops
        return [ops.MapRows(*[self._buf[k][b] if k in attrs and self._buf[k] is not None else None for k in _ATTRS],
                            *self._count_of(b)) for b in range(len(self._n_host))]

    def _row_outs(self, maps, dtype, want):
        """per sequence an empty (bound,) output of a pass that marks rows (ops._seq_outs), None where not wanted"""
        return [torch.empty(min(m.n_bound, int(m.points.shape[0])), dtype=dtype, device=self.device) if want else None
                for m in maps]

    def _tighten_counts(self):
        """Reads the device-side counts back (one sync) and makes the host-side BOUNDS exact, keeping the device counts in
        charge: the next step takes the same path as without this call (used by profiling passes, whose byte counts come
        from the bounds)."""
        if not self._dcount:
            return list(self._n_host)
        for grp in {id(dc.group): dc.group for dc in self._dcount.values()}.values():
            grp.tighten()
        return [self._dcount[b].bound if b in self._dcount else self._n_host[b] for b in range(len(self._n_host))]

    def _set_count_dev(self, b, dev_count, max_growth):
        """The kernels wrote the new count of sequence b to `dev_count`; at most `max_growth` rows
        were added.  Nothing is read back (see _DeviceCount)."""
        dc = self._dcount.get(b)
        if dc is None or len(dc.group.bounds) != 1:
            bound = (self._n_host[b] if dc is None else dc.bound) + int(max_growth)
            self._dcount[b] = _DeviceCount(_CountGroup(dev_count.reshape(1), [bound]), 0)
        else:
            dc.group.advance(dev_count.reshape(1), max_growth)
        self._generation += 1
        self._padded_cache.clear()
        self.equisized = True if len(self._n_host) == 1 else None

    def _set_counts_dev(self, dev_counts, max_growth):
        """Same for every sequence of the batch at once: dev_counts is the (B,) int64 tensor the batched kernels
        wrote; ONE asynchronous read-back serves all sequences."""
        B = len(self._n_host)
        dcs = [self._dcount.get(b) for b in range(B)]
        grp = dcs[0].group if dcs[0] is not None else None
        if grp is not None and len(grp.bounds) == B and all(d is not None and d.group is grp and d.index == b
                                                            for b, d in enumerate(dcs)):
            grp.advance(dev_counts, max_growth)
        else:
            bounds = [(self._n_host[b] if d is None else d.bound) + int(max_growth) for b, d in enumerate(dcs)]
            grp = _CountGroup(dev_counts, bounds)
            for b in range(B):
                self._dcount[b] = _DeviceCount(grp, b)
        self._generation += 1
        self._padded_cache.clear()
        self.equisized = True if B == 1 else None

    # ------------------------------------------------------------------ feature layers
    def attach_features(self, layer):
        r"""Attaches a `MapFeatures` layer: from now on `PointFusion.step(..., inplace=True, features=...)` fuses
        per-pixel feature images into it with the weights and the correspondences of the colour fusion, and `prune_`,
        `carve_`, `voxel_downsample_` and the drivers' schedules keep it row-aligned with the map.  The rows a non-empty
        map already holds get zeros with weight 0.  A layer belongs to one map object: `clone()`, indexing and the
        out-of-place `prune` / `carve` / `voxel_downsample` return maps without it.  `append_points`, the attribute
        setters and `ICPSLAM.step` refuse a map with a layer (they would change rows behind its back).  Returns self."""
        from .mapfeatures import MapFeatures
        if not isinstance(layer, MapFeatures):
            raise TypeError("Expected layer to be of type gradslam.MapFeatures. Got {0}.".format(type(layer)))
        if self._feature_layer is not None:
            raise ValueError("this pointclouds object already has a feature layer (detach_features() first)")
        if layer._map is not None:
            raise ValueError("the feature layer is attached to another pointclouds object: a layer belongs to one map")
        layer._emb = layer._weight = None
        layer._map = self
        self._feature_layer = layer
        if len(self._n_host):
            layer._bind(self)
        return self

    @property
    def map_features(self):
        """the attached `MapFeatures` layer, or None"""
        return self._feature_layer

    def detach_features(self):
        """Takes the feature layer off the map and returns it (None when there is none).  The layer keeps its buffers,
        but no longer follows the map: its list views are gone until it is attached again (which starts it afresh)."""
        layer = self._feature_layer
        if layer is not None:
            layer._map = None
        self._feature_layer = self._fuse_record = None
        return layer

    def _refuse_with_features(self, what):
        if self._feature_layer is not None:
            raise ValueError("{} is not supported on a map with a feature layer attached: the layer's rows would no "
                             "longer belong to the map's (detach_features() first)".format(what))

    # ------------------------------------------------------------------ the model view
    def render(self, intrinsics: torch.Tensor, poses: torch.Tensor, height: int, width: int, *, radius: int = 0,
               min_confidence: float = 0.0, cull_backfaces: bool = False, return_extras: bool = False,
               differentiable: bool = False, radii=None, max_radius: int = 3):
        r"""The map seen from camera poses: a z-buffered point render (HIP; the result is detached unless
        `differentiable` is set).

        Every point competes for the pixel it projects to (the projection of the SLAM association, with the image size
        `height` x `width`, which need not be the capture size -- scale the intrinsics to match); the nearest point
        wins, the lowest row index among points at bit-equal depth.  Pixels no point lands on hold depth 0 / colour 0.

        Args:
            intrinsics: (B, 1, 4, 4), as in `RGBDImages`
            poses: (B, L, 4, 4) camera-to-world
            radius: 0..3; a point competes for the (2 radius + 1)^2 pixel square around its pixel (closes the holes of
                a view that is nearer than the capture)
            radii: per-surfel splat sizes instead of one `radius` (which must then be 0).  "layer": the radii of the
                attached `SurfelRadii` layer; or a list of B (N_b,) float32 tensors, radii in metres.  A point of
                radius rho at depth z in a view competes for the square of half-width min(max_radius, floor(rho fbar /
                z)), fbar the mean focal length of `intrinsics`: about one pixel-footprint of the sample it was fused
                from, so a nearer view closes its holes and a farther one does not fatten.  A radius that is 0,
                negative, NaN or inf splats one pixel.  Constants of the gradient.
            max_radius: 0..8, the cap of that half-width
            min_confidence: points whose confidence count (the first and only feature channel) is below it are skipped
            cull_backfaces: points whose normal n has n.q >= 0 at their camera-frame position q (facing away from the
                camera, or edge-on) are skipped.  Mind the orientation of the map's normals: the frame normals of
                `RGBDImages` (and of the reference) mostly point away from the camera that saw them, so on a map fused
                from them this removes the visible side
            return_extras: also return {"normal": (B, L, H, W, 3) camera-frame normal of the winner, "confidence":
                (B, L, H, W, 1), "index": (B, L, H, W) int64 row of the winner or -1}
            differentiable: keep the rendered depth, colour, normal and confidence on the autograd tape
                (`ops.RenderMapFunction`, a HIP backward kernel): a loss on them reaches the map buffers and `poses`,
                neither of which is detached.  The z-buffer is hard: which point wins a pixel, and the two filters, are
                constants of the gradient; `intrinsics` and the index image get none.  The backward pass re-projects
                the map, so run it before the map is changed in place (before the next `PointFusion.step`); a
                backward after such a change raises instead of returning gradients of the wrong rows.

        Returns:
            RGBDImages of shape (B, L, height, width) holding the rendered colour and depth with `intrinsics` and
            `poses` (and the extras dict with `return_extras`).

        The map buffers are only read: counts that live on the device stay there, nothing is reallocated."""
        from .. import ops
        from .rgbdimages import RGBDImages
        for name, val in (("intrinsics", intrinsics), ("poses", poses)):
            if not torch.is_tensor(val):
                raise TypeError("Expected {} to be of type tensor; got {}".format(name, type(val)))
        B = len(self)
        if B == 0 or self._buf["points"] is None:
            raise ValueError("cannot render an empty pointclouds object")
        if any(self._buf[k] is None for k in ("normals", "colors", "features")) or self.num_features != 1:
            raise ValueError("render needs a surfel map: points, normals, colors and one feature channel (confidence)")
        if poses.ndim != 4 or tuple(poses.shape[2:]) != (4, 4) or poses.shape[0] != B or poses.shape[1] == 0:
            raise ValueError("poses should have shape ({}, L, 4, 4), but had shape {}".format(B, tuple(poses.shape)))
        if tuple(intrinsics.shape) != (B, 1, 4, 4):
            raise ValueError("intrinsics should have shape {}, but had shape {}".format((B, 1, 4, 4),
                                                                                     tuple(intrinsics.shape)))
        if radii is not None and not isinstance(radii, str):
            # a caller's tensors are sized by the counts: make the host-side bounds exact (one read-back; the device
            # counts stay in charge), before the guard below takes its snapshot of the map
            self._tighten_counts()
        guard = None
        if differentiable:
            generation = self._generation

            def guard():
                if self._generation != generation:
                    raise RuntimeError("the map was changed in place after render(differentiable=True) and before its "
                                       "backward pass: the saved winners no longer belong to the map rows (run backward "
                                       "before the next PointFusion.step, or render again)")
        maps = self._map_rows()
        if isinstance(radii, str):
            from .mapfeatures import SurfelRadii
            if radii != "layer":
                raise ValueError("radii must be None, 'layer' or a list of (N_b,) float32 tensors; got {!r}".format(radii))
            layer = self._feature_layer
            if not isinstance(layer, SurfelRadii) or layer._emb is None:
                raise ValueError("radii='layer' needs a SurfelRadii layer on the map (attach_features(SurfelRadii()), or "
                                 "PointFusion(surfel_radii=True)); pass the radii as a list otherwise")
            radii = [layer._emb[b][:min(m.n_bound, int(m.points.shape[0])), 0] for b, m in enumerate(maps)]
        out = ops.render_map_batch(maps, poses, intrinsics[:, 0], int(height), int(width), radius=radius,
                                   min_confidence=min_confidence, cull_backfaces=cull_backfaces,
                                   differentiable=differentiable, guard=guard, radii=radii, max_radius=max_radius)
        frames = RGBDImages(out.color, out.depth, intrinsics.detach().to(torch.float32),
                            poses.to(torch.float32) if differentiable else poses.detach().to(torch.float32))
        if return_extras:
            return frames, {"normal": out.normal, "confidence": out.confidence, "index": out.index}
        return frames

    # ------------------------------------------------------------------ pruning
    # Rows are appended after all older rows and a prune keeps their order, so the index of a row is monotone in the step
    # that created it: "appended since epoch e" is "row >= the count at e".  The map remembers the counts of its last
    # MAX_MARKS epochs (the marks); a prune rewrites each mark as the number of survivors in front of it.
    MAX_MARKS = 64

    def _carry_epochs(self, other, ids=None):
        """takes the epoch marks and the step counter of `other` (of its sequences `ids`)"""
        self._prune_steps = other._prune_steps
        self._carve_steps = other._carve_steps
        self._voxel_steps = other._voxel_steps
        self._n_marks = other._n_marks if other._marks is not None else 0
        if other._marks is None:
            self._marks = None
        else:
            self._marks = (other._marks if ids is None else other._marks[ids]).clone().to(self.device)

    def _count_group(self):
        """the _CountGroup that holds the device-side counts of ALL sequences, in order, or None"""
        B = len(self._n_host)
        dc = self._dcount
        if B == 0 or len(dc) != B:
            return None
        g0 = dc[0].group
        if len(g0.bounds) != B or any(dc[b].group is not g0 or dc[b].index != b for b in range(B)):
            return None
        return g0

    def mark_epoch(self):
        r"""Records the current counts as the newest epoch mark (at most `MAX_MARKS` are kept, the oldest is dropped).
        `prune_(..., min_age=k)` protects the rows appended since the k-th newest mark.  Counts that live on the device are
        copied device-to-device: nothing is read back."""
        B = len(self._n_host)
        if B == 0:
            return self
        if self._marks is None or self._marks.shape[0] != B or self._marks.device != self.device:
            self._marks = torch.zeros((B, self.MAX_MARKS), dtype=torch.int64, device=self.device)
            self._n_marks = 0
        if self._n_marks == self.MAX_MARKS:
            self._marks[:, :-1] = self._marks[:, 1:].clone()
            self._n_marks -= 1
        k = self._n_marks
        grp = self._count_group()
        if grp is not None:
            self._marks[:, k].copy_(grp.dev)
        elif self._dcount:
            for b in range(B):
                dc = self._dcount.get(b)
                if dc is not None:
                    self._marks[b, k:k + 1].copy_(dc.dev)
                else:
                    self._marks[b, k] = self._n_host[b]
        else:
            self._marks[:, k] = torch.tensor(self._n_host, dtype=torch.int64)
        self._n_marks = k + 1
        return self

    def _keep_list(self, keep):
        B = len(self._n_host)
        if keep is None:
            return [None] * B
        if torch.is_tensor(keep):
            if keep.ndim != 2 or keep.shape[0] != B:
                raise ValueError("keep should have shape ({}, N), but had shape {}".format(B, tuple(keep.shape)))
            keep = [keep[b] for b in range(B)]
        elif not isinstance(keep, list):
            raise TypeError("Expected keep to be of type list or tensor or None; got %r" % type(keep))
        if len(keep) != B:
            raise ValueError("keep must have one entry per pointcloud. Got {} != {}.".format(len(keep), B))
        for t in keep:
            if not torch.is_tensor(t) or t.ndim != 1 or t.dtype not in (torch.bool, torch.uint8):
                raise TypeError("keep must hold 1-d bool / uint8 tensors, one per pointcloud")
        return [t.to(self.device) for t in keep]

    def prune_(self, min_confidence: Optional[float] = None, *, keep=None, min_age: int = 0):
        r"""Removes rows in place, keeping the order of the rest.  Row r of a sequence survives iff

            (keep is None or keep[r] != 0) and (min_confidence is None or r is young or confidence[r] >= min_confidence)

        (float32 compare: a NaN confidence is removed, a confidence equal to the threshold stays).

        Args:
            min_confidence: threshold on the confidence count (the first and only feature channel of a surfel map)
            keep: list of (N_b,) bool / uint8 tensors, or a (B, N) tensor; rows beyond a sequence's tensor are removed
            min_age: k > 0 protects ("young") the rows appended since the k-th newest `mark_epoch()` from the confidence
                rule; with fewer than k marks recorded every row is young.  0 protects nothing.

        On a HIP device this is one batched compaction (gs_prune_map_dc_f32) into new buffers of the same capacity;
        counts that live on the device stay there (nothing is read back; the host-side bounds tighten with the next
        read-back that lands).  `last_pruned` holds the removed rows per sequence.  Returns self."""
        B = len(self._n_host)
        if B == 0 or self._buf["points"] is None:
            raise ValueError("cannot prune an empty pointclouds object")
        if not (min_confidence is None or isinstance(min_confidence, (float, int))):
            raise TypeError("min_confidence must be of type float or int or None; but was of type {}.".format(
                type(min_confidence)))
        if not isinstance(min_age, int) or isinstance(min_age, bool) or min_age < 0:
            raise ValueError("min_age must be a non-negative int; got {!r}".format(min_age))
        if min_confidence is not None and (any(self._buf[k] is None for k in ("normals", "colors", "features")) or
                                           self.num_features != 1):
            raise ValueError("prune needs a surfel map: points, normals, colors and one feature channel (confidence)")
        keep = self._keep_list(keep)
        conf, young_mark = min_confidence, -1
        if conf is not None and min_age > 0:
            n_marks = self._n_marks if self._marks is not None else 0
            if n_marks < min_age:
                conf = None          # every row is young: the confidence rule removes nothing
            else:
                young_mark = n_marks - min_age
        taped = torch.is_grad_enabled() and any(t.requires_grad for k in _ATTRS if self._buf[k] is not None
                                                for t in self._buf[k])
        f32 = all(t.dtype == torch.float32 for k in _ATTRS if self._buf[k] is not None for t in self._buf[k])
        if conf is None and all(k is None for k in keep):
            self.last_pruned = torch.zeros(B, dtype=torch.int64, device=self.device)
        elif self.device.type == "cuda" and f32 and not taped:
            if self._feature_layer is not None:
                # the rule as an explicit mask, formed on the device: the map and the layer are compacted by the same one
                keep, conf, young_mark = self._explicit_keep(conf, keep, young_mark), None, -1
            self._prune_hip(conf, keep, young_mark)
        else:
            self._prune_torch(conf, keep, young_mark)
        self._generation += 1
        self._padded_cache.clear()
        return self

    def prune(self, min_confidence: Optional[float] = None, *, keep=None, min_age: int = 0):
        r"""Out-of-place `prune_`: returns a pruned copy (the copy resolves device-side counts, as `clone` does)."""
        return self.clone().prune_(min_confidence, keep=keep, min_age=min_age)

    # ------------------------------------------------------------------ free-space carving
    def _free_space(self, who, frames, margin, window, min_views, want):
        """ops.free_space_batch of the map, read in place with its device-side counts, against all frames of `frames`;
        want: (violations, keep)"""
        from .. import ops
        from .rgbdimages import RGBDImages
        if not isinstance(frames, RGBDImages):
            raise TypeError("Expected frames to be of type gradslam.RGBDImages. Got {0}.".format(type(frames)))
        margin, window, min_views = ops._carve_args(who, margin, window, min_views)
        B = len(self._n_host)
        if B == 0 or self._buf["points"] is None:
            raise ValueError("cannot carve an empty pointclouds object")
        if frames.poses is None:
            raise ValueError("{} needs frames with poses".format(who))
        if frames.shape[0] != B:
            raise ValueError("frames must hold one sequence per pointcloud. Got {} != {}.".format(frames.shape[0], B))
        d = frames.depth_image
        d = d[:, :, 0] if frames.channels_first else d[..., 0]   # (B, L, H, W), a view: one channel either way
        maps = self._map_rows(("points",))
        out = (self._row_outs(maps, torch.int32, want[0]), self._row_outs(maps, torch.uint8, want[1]))
        return ops.free_space_batch(maps, d, frames.poses, frames.intrinsics[:, 0], margin=margin, window=window,
                                    min_views=min_views, out=out)

    def free_space_violations(self, frames, *, margin: float = 0.05, window: int = 1):
        r"""Per sequence the (N_b,) int32 number of frames of `frames` (an `RGBDImages` of shape (B, L, H, W) with poses)
        that see through each point: the point projects into the frame (the projection of the map update and of
        `render`), its pixel has depth, and every pixel with depth of the (2 window + 1)^2 square around it measures
        more than `margin` behind the point (`ops.free_space_batch`; HIP, detached).  The map is only read, with its
        device-side counts: it can be called between steps; rows the host-side bound holds beyond a device-side count
        read 0."""
        return self._free_space("free_space_violations", frames, margin, window, 1, (True, False)).violations

    def carve_(self, frames, *, margin: float = 0.05, window: int = 1, min_views: int = 1):
        r"""Free-space carving in place: removes the points that at least `min_views` frames of `frames` see through
        (`free_space_violations`), keeping the order of the rest.  No confidence rule is applied.  The removal is
        `prune_(keep=...)` with the mask the carve kernel wrote: counts stay on the device, the epoch marks are
        rewritten, `last_pruned` holds the removed rows, and a differentiable render or projective-ICP solve taken before
        it refuses a late backward, as for `prune_`.  A map on the autograd tape takes `prune_`'s torch path with the
        (detached) mask.  Returns self."""
        keep = self._free_space("carve_", frames, margin, window, min_views, (False, True)).keep
        return self.prune_(None, keep=keep)

    def carve(self, frames, *, margin: float = 0.05, window: int = 1, min_views: int = 1):
        r"""Out-of-place `carve_`: returns a carved copy (the copy resolves device-side counts, as `clone` does)."""
        return self.clone().carve_(frames, margin=margin, window=window, min_views=min_views)

    # ------------------------------------------------------------------ voxel thinning
    def _voxel_keep(self, who, voxel_size, want):
        """the voxel rule on the map, read in place with its device-side counts; want: (keep, winner).  Returns the two
        per-sequence lists (None where not wanted).  A float32 map on a HIP device goes through ops.voxel_keep_batch;
        any other map (CPU, another dtype) through the same rule in torch (_voxel_keep_torch)."""
        from .. import ops
        voxel_size = ops._voxel_args(who, voxel_size)
        B = len(self._n_host)
        if B == 0 or self._buf["points"] is None:
            raise ValueError("cannot voxel-downsample an empty pointclouds object")
        # the confidence competes only on a surfel map's single count channel; any other feature layout scores 0
        conf = self._buf["features"] if self._buf["features"] is not None and self.num_features == 1 else None
        pts = self._buf["points"]
        if self.device.type == "cuda" and all(t.dtype == torch.float32 for t in pts) and \
                (conf is None or all(t.dtype == torch.float32 for t in conf)):
            # (detached: the mask is a constant, and the pass need not say so)
            maps = [m._replace(points=m.points.detach(), features=None if conf is None else m.features.detach())
                    for m in self._map_rows(("points", "features"))]
            r = ops.voxel_keep_batch(maps, voxel_size, out=(self._row_outs(maps, torch.uint8, want[0]),
                                                            self._row_outs(maps, torch.int64, want[1])))
            return r.keep, r.winner
        keep, winner = [], []
        for b, nb in enumerate(self._n):
            k, w = _voxel_keep_torch(pts[b][:nb].detach(), None if conf is None else conf[b][:nb, 0].detach(), voxel_size)
            keep.append(k if want[0] else None)
            winner.append(w if want[1] else None)
        return keep, winner

    def voxel_winners(self, voxel_size: float):
        r"""Per sequence the (N_b,) int64 row of the surfel that the voxel of each point keeps: the most confident point
        of the cube of side `voxel_size` that holds it (voxel index floor(p / voxel_size) per component, in float32),
        the oldest among equals; the point itself where it cannot be put on the grid (a non-finite coordinate, a voxel
        index outside [-2^20, 2^20)).  The confidence is the single feature channel of a surfel map; a map with another
        feature layout scores every point 0 (the first point of a voxel wins).  `index_add` over it averages attributes
        per voxel.  The map is only read, with its device-side counts: it can be called between steps; rows the
        host-side bound holds beyond a device-side count read -1."""
        return self._voxel_keep("voxel_winners", voxel_size, (False, True))[1]

    def voxel_downsample_(self, voxel_size: float):
        r"""Voxel thinning in place: keeps one point per cube of side `voxel_size` -- the winner of `voxel_winners` --
        and every point that cannot be put on the grid, keeping the order of the rest.  Nothing is averaged or moved.
        The removal is `prune_(keep=...)` with the mask of the voxel pass: counts stay on the device, the epoch marks
        are rewritten, `last_pruned` holds the removed rows, and a differentiable render or projective-ICP solve taken
        before it refuses a late backward, as for `prune_`.  A map on the CPU or on the autograd tape takes `prune_`'s
        torch path with the (detached) mask: the kept rows stay on the tape.  A second call removes nothing.  Returns
        self."""
        keep = self._voxel_keep("voxel_downsample_", voxel_size, (True, False))[0]
        return self.prune_(None, keep=keep)

    def voxel_downsample(self, voxel_size: float):
        r"""Out-of-place `voxel_downsample_`: returns a thinned copy (the copy resolves device-side counts, as `clone`
        does)."""
        from .. import ops
        ops._voxel_args("voxel_downsample", voxel_size)
        return self.clone().voxel_downsample_(voxel_size)

    def _explicit_keep(self, conf, keep, young_mark):
        """prune_'s rule over the host-side bound of every sequence as uint8 masks: (row >= marks[young_mark]) |
        (confidence >= float32(min_confidence)), AND-ed with the caller's mask (rows it does not cover are removed).
        Elementwise torch on the device, nothing is read back; a NaN confidence fails, as in the kernel."""
        out = []
        for b in range(len(self._n_host)):
            bound = self._count_of(b)[0]
            s = torch.ones(bound, dtype=torch.bool, device=self.device)
            if keep[b] is not None:
                kp = keep[b][:bound] != 0
                s[: kp.shape[0]] &= kp
                s[kp.shape[0]:] = False
            if conf is not None:
                cc = self._buf["features"][b][:bound, 0]
                ok = cc >= torch.tensor(conf, dtype=torch.float32, device=self.device)
                if young_mark >= 0:
                    ok |= torch.arange(bound, device=self.device) >= self._marks[b, young_mark]
                s &= ok
            out.append(s.to(torch.uint8))
        return out

    def _prune_hip(self, conf, keep, young_mark):
        from .. import ops
        B = len(self._n_host)
        maps, keeps = self._map_rows(), []
        for b, bound in enumerate(m.n_bound for m in maps):
            kp = keep[b]
            if kp is not None and kp.shape[0] < bound:   # (rows the caller's tensor does not cover are removed)
                kp = torch.cat([kp.to(torch.uint8), torch.zeros(bound - kp.shape[0], dtype=torch.uint8, device=kp.device)])
            keeps.append(kp)
        n_marks = self._n_marks if self._marks is not None else 0
        marks = [self._marks[b, :n_marks] for b in range(B)] if n_marks else None
        r = ops.prune_map_batch(maps, min_confidence=conf, keep=keeps if any(k is not None for k in keeps) else None,
                                marks=marks, young_mark=young_mark)
        for b in range(B):
            for i, k in enumerate(_ATTRS):
                if self._buf[k] is not None:
                    self._buf[k][b] = r.maps[b][i]     # same capacity: nothing that follows the capacity is re-sized
        if self._feature_layer is not None:
            # (the counts of `maps` are those from before the prune: the layer's rows are the map's rows)
            self._feature_layer._compact([(m.n_bound, m.n_dev) for m in maps], keeps)
        grp = self._count_group()
        if grp is not None:
            grp.shrink(r.counts)
            self.equisized = True if B == 1 else None
        else:
            self._n = [int(v) for v in r.counts.tolist()]     # host-side counts: one read-back
            self.equisized = len(set(self._n_host)) == 1
        self.last_pruned = r.removed

    def _prune_torch(self, conf, keep, young_mark):
        """the same rule through boolean indexing (CPU maps, maps on the autograd tape: the kept rows stay on it)"""
        n = self._n
        n_marks = self._n_marks if self._marks is not None else 0
        new_n, removed = [], []
        for b, nb in enumerate(n):
            s = torch.ones(nb, dtype=torch.bool, device=self.device)
            if keep[b] is not None:
                kp = keep[b][:nb] != 0
                s[: kp.shape[0]] &= kp
                s[kp.shape[0]:] = False
            if conf is not None:
                cc = self._buf["features"][b][:nb, 0].detach().to(torch.float32)
                passes = cc >= torch.tensor(conf, dtype=torch.float32, device=self.device)
                if young_mark >= 0:
                    passes |= torch.arange(nb, device=self.device) >= self._marks[b, young_mark]
                s &= passes
            for k in _ATTRS:
                if self._buf[k] is not None:
                    self._buf[k][b] = self._buf[k][b][:nb][s]
            if self._feature_layer is not None:
                self._feature_layer._select(b, nb, s)
            if n_marks:
                before = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(s, 0)])
                self._marks[b, :n_marks] = before[self._marks[b, :n_marks].clamp(0, nb)]
            kept = int(s.sum())
            new_n.append(kept)
            removed.append(nb - kept)
        self._n = new_n
        self.equisized = len(set(new_n)) == 1
        self.last_pruned = torch.tensor(removed, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ copies / moves
    def clone(self):
        other = Pointclouds(device=self.device)
        other._n = list(self._n)
        for k in _ATTRS:
            other._buf[k] = None if self._buf[k] is None else [t[:n].clone() for t, n in zip(self._buf[k], self._n)]
        other.equisized = self.equisized
        other._carry_epochs(self)
        return other

    def detach(self):
        other = Pointclouds(device=self.device)
        other._n = list(self._n)
        for k in _ATTRS:
            other._buf[k] = None if self._buf[k] is None else [t.detach() for t in self._buf[k]]
        other.equisized = self.equisized
        other._carry_epochs(self)
        return other

    def to(self, device, copy: bool = False):
        device = _canon_device(device)
        if not copy and self.device == device:
            return self
        other = self.clone()
        if self.device != device:
            other.device = device
            for k in _ATTRS:
                if other._buf[k] is not None:
                    other._buf[k] = [t.to(device) for t in other._buf[k]]
            if other._marks is not None:
                other._marks = other._marks.to(device)
        return other

    def cpu(self):
        return self.to(torch.device("cpu"))

    def cuda(self):
        return self.to(torch.device("cuda"))

    # ------------------------------------------------------------------ append
    def append_points(self, pointclouds: "Pointclouds"):
        r"""Appends the points of `pointclouds` sequence-wise, in place
        (reference: structures/pointclouds.py:1117-1237)."""
        if not isinstance(pointclouds, type(self)):
            raise TypeError("Append object must be of type gradslam.Pointclouds, but was of type {}.".format(
                type(pointclouds)))
        if not (pointclouds.device == self.device):
            raise ValueError("Device of pointclouds to append and to be appended must match: ({0} != {1})".format(
                pointclouds.device, self.device))
        self._refuse_with_features("append_points")
        if not pointclouds.has_points:
            return self
        if self.has_points:
            if len(pointclouds) != len(self):
                raise ValueError("Batch size of pointclouds to append and to be appended must match: ({0} != {1})"
                                 .format(len(pointclouds), len(self)))
            for name in ("normals", "colors", "features"):
                if (self._buf[name] is not None) != (pointclouds._buf[name] is not None):
                    raise ValueError("pointclouds to append and to be appended must either both have or not have "
                                     "{0}: ({1} != {2})".format(name, pointclouds._buf[name] is not None,
                                                                self._buf[name] is not None))
            if self.has_features and self.num_features != pointclouds.num_features:
                raise ValueError("pointclouds to append and to be appended must have the same number of features: "
                                 "({0} != {1})".format(pointclouds.num_features, self.num_features))
            for b in range(len(self)):
                m = pointclouds._n[b]
                if m == 0:
                    continue
                self._reserve(b, m)
                n0 = self._n[b]
                for k in _ATTRS:
                    if self._buf[k] is not None:
                        self._buf[k][b][n0:n0 + m] = pointclouds._buf[k][b][:m]
                self._n[b] = n0 + m
        else:
            self._n = list(pointclouds._n)
            for k in _ATTRS:
                src = pointclouds._buf[k]
                self._buf[k] = None if src is None else [t[:n].clone() for t, n in zip(src, pointclouds._n)]
        self._invalidate()
        return self

    # ------------------------------------------------------------------ rigid-body helpers
    # Container algebra of the reference API (pointclouds.py:399-614).  The SLAM hot path does
    # NOT go through these (projection/association is fused in the HIP kernels).
    def _apply(self, k, fn):
        if self._buf[k] is not None:   # (results land on capacity-backed buffers again: _store_rows)
            self._store_rows(k, [fn(b, t[:n]) for b, (t, n) in enumerate(zip(self._buf[k], self._n))])

    @staticmethod
    def _rigid_rows(t, M, tvec=None):
        """t @ M (+ tvec) for the rows of one cloud.  On the GPU: gs_transform_points_f32 (the FMA chain of the
        reference's batched matmul, then the translation); on the CPU (host-side logic, tests): the same as tensor ops."""
        if t.is_cuda and t.dtype == torch.float32 and not t.requires_grad:
            from .. import ops
            T = torch.zeros((4, 4), dtype=torch.float32, device=t.device)
            T[:3, :3] = M.transpose(0, 1)
            if tvec is not None:
                T[:3, 3] = tvec
            T[3, 3] = 1.0
            return ops.transform_points(t, T)
        out = t @ M
        return out if tvec is None else out + tvec

    def offset_(self, offset):
        if not (torch.is_tensor(offset) or isinstance(offset, (float, int))):
            raise TypeError("Operand should be tensor, float or int but was %r instead" % type(offset))
        if not self.has_points:
            return self
        if torch.is_tensor(offset) and offset.ndim == 3:
            self._apply("points", lambda b, t: t + offset[b if offset.shape[0] > 1 else 0, : t.shape[0] if offset.shape[1] > 1 else 1])
        else:
            self._apply("points", lambda b, t: t + offset)
        return self

    def scale_(self, scale):
        if not (torch.is_tensor(scale) or isinstance(scale, (float, int))):
            raise TypeError("Operand should be tensor, float or int but was %r instead" % type(scale))
        if self.has_points:
            self._apply("points", lambda b, t: t * scale)
        return self

    def rotate_(self, rmat: torch.Tensor, *, pre_multiplication=True):
        if not torch.is_tensor(rmat):
            raise TypeError("Rotation matrix should be tensor, but was %r instead" % type(rmat))
        if not ((rmat.ndim == 2 or rmat.ndim == 3) and rmat.shape[-2:] == (3, 3)):
            raise ValueError("Rotation matrix should be of shape (3, 3) or (B, 3, 3), but was {} instead.".format(
                rmat.shape))
        if rmat.ndim == 3 and rmat.shape[0] != len(self):
            raise ValueError("Rotation matrix batch size ({}) != Pointclouds batch size ({})".format(
                rmat.shape[0], len(self)))
        if not self.has_points:
            return self
        if pre_multiplication:
            rmat = rmat.transpose(-1, -2)
        pick = (lambda b: rmat[b]) if rmat.ndim == 3 else (lambda b: rmat)
        self._apply("points", lambda b, t: self._rigid_rows(t, pick(b)))
        self._apply("normals", lambda b, t: self._rigid_rows(t, pick(b)))
        return self

    def transform_(self, transform: torch.Tensor, *, pre_multiplication=True):
        if not torch.is_tensor(transform):
            raise TypeError("transform should be tensor, but was %r instead" % type(transform))
        if not ((transform.ndim == 2 or transform.ndim == 3) and transform.shape[-2:] == (4, 4)):
            raise ValueError("transform should be of shape (4, 4) or (B, 4, 4), but was {} instead.".format(
                transform.shape))
        if transform.ndim == 3 and transform.shape[0] != len(self):
            raise ValueError("transform batch size ({}) != Pointclouds batch size ({})".format(
                transform.shape[0], len(self)))
        if not self.has_points:
            return self
        rmat, tvec = transform[..., :3, :3], transform[..., :3, 3]
        self.rotate_(rmat, pre_multiplication=pre_multiplication)
        pick = (lambda b: tvec[b]) if tvec.ndim == 2 else (lambda b: tvec)
        self._apply("points", lambda b, t: t + pick(b))
        return self

    def pinhole_projection_(self, intrinsics: torch.Tensor):
        if not torch.is_tensor(intrinsics):
            raise TypeError("intrinsics should be tensor, but was {} instead".format(type(intrinsics)))
        if not ((intrinsics.ndim == 2 or intrinsics.ndim == 3) and intrinsics.shape[-2:] == (4, 4)):
            raise ValueError("intrinsics should be of shape (4, 4) or (B, 4, 4), but was {} instead.".format(
                intrinsics.shape))
        if not self.has_points:
            return self
        pick = (lambda b: intrinsics[b]) if intrinsics.ndim == 3 else (lambda b: intrinsics)

        def proj(b, t):
            K = pick(b)
            if t.is_cuda and t.dtype == torch.float32 and not t.requires_grad:   # gs_project_points_f32
                from .. import ops
                uv = ops.project_points(t, K.reshape(1, 4, 4), max(int(t.shape[0]), 1))
                return torch.cat([uv, torch.ones_like(uv[:, :1])], -1)
            h = torch.cat([t, torch.ones_like(t[:, :1])], -1) @ K.transpose(0, 1)
            z = torch.where(h[:, 2:3] != 0, h[:, 2:3], torch.ones_like(h[:, 2:3]))
            return torch.cat([h[:, :2] / z, torch.ones_like(z)], -1)

        self._apply("points", proj)
        return self

    # arithmetic operators of the reference (structures/pointclouds.py:300-384): out-of-place offset / scale /
    # rotation / rigid transform
    def __add__(self, other):
        try:
            return self.clone().offset_(other)
        except TypeError:
            raise NotImplementedError("Pointclouds + {} currently not implemented.".format(type(other)))

    def __sub__(self, other):
        try:
            return self.clone().offset_(other * -1)
        except TypeError:
            raise NotImplementedError("Pointclouds - {} currently not implemented.".format(type(other)))

    def __mul__(self, other):
        try:
            return self.clone().scale_(other)
        except TypeError:
            raise NotImplementedError("Pointclouds * {} currently not implemented.".format(type(other)))

    def __truediv__(self, other):
        try:
            return self.__mul__(1.0 / other)
        except TypeError:
            raise NotImplementedError("Pointclouds / {} currently not implemented.".format(type(other)))

    def __matmul__(self, other):
        if not torch.is_tensor(other):
            raise NotImplementedError("Pointclouds @ {} currently not implemented.".format(type(other)))
        if not ((other.ndim == 2 or other.ndim == 3) and (other.shape[-2:] == (3, 3) or other.shape[-2:] == (4, 4))):
            msg = "Unsupported shape for Pointclouds @ operand: {}\n".format(other.shape)
            msg += "Use tensor of shape (3, 3) or (B, 3, 3) for rotations, or (4, 4) or (B, 4, 4) for transformations"
            raise ValueError(msg)
        if other.shape[-2:] == (3, 3):
            return self.clone().rotate_(other, pre_multiplication=False)
        return self.clone().transform_(other, pre_multiplication=False)

    def offset(self, offset):
        return self.clone().offset_(offset)

    def scale(self, scale):
        return self.clone().scale_(scale)

    def rotate(self, rmat, *, pre_multiplication=True):
        return self.clone().rotate_(rmat, pre_multiplication=pre_multiplication)

    def transform(self, transform, *, pre_multiplication=True):
        return self.clone().transform_(transform, pre_multiplication=pre_multiplication)

    def pinhole_projection(self, intrinsics):
        return self.clone().pinhole_projection_(intrinsics)
