"""Which K frames of a recorded drive to label: greedy k-center selection in feature space.

The reference's README ends its campus-map section with two remedies, domain adaptation or targeted
data collection.  ``FeatureDensity`` / ``Predictor.predict_novelty`` say how far ONE frame is from
what the trunk saw in training; the top-K novel frames of a 20 Hz log are a few hundred near-copies
of the same junction.  The core-set rule (Sener & Savarese, 2018) starts from what is already
covered and repeatedly takes the frame farthest from everything chosen so far; it is defined in
include/cilrs_hip.h ("Greedy k-center") and runs as one streaming pass over the pool per pick
(csrc/kcenter.hip).  The same call thins a redundant training set.

    pool = FramePool(model, capacity=200_000)
    for images, speeds, commands in log_batches:        # eval-mode forwards, nothing copied to the host
        pool.add(images, speeds, commands)
    s = pool.select(500, density=fd)                    # Mahalanobis metric, the fit's command means covered
    s.indices, s.coverage()                             # frames to label; covering radius after each pick
    more = pool.select(500, density=fd, covered=pool.features()[torch.from_numpy(s.indices).cuda()])
    idx, dist = pool.index(density=fd).query(features, k=8)     # the nearest recorded frames

fp32 only: the pool goes through the module's fp32 eval-mode forward.  There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L


@dataclass
class Selection:
    """indices int64 [k'] and radius float32 [k'] on the host: radius[t] is the squared distance of
    pick t to everything covered before it, non-increasing; the picks are cut at the first
    radius == 0 (every remaining row coincides with a chosen one), so k' <= k.  min_dist float32
    [N] (device): each pool row's squared distance to the nearest centre after the last pick.  rows:
    the device rows the selection ran on (the whitened pool, or the pool itself)."""
    indices: np.ndarray
    radius: np.ndarray
    min_dist: torch.Tensor
    metric: str
    rows: torch.Tensor = None

    def coverage(self):
        """The covering radius after each pick, in the metric's own unit: the curve to read "how
        many frames are enough" from."""
        return np.sqrt(self.radius)


class FramePool:
    """Pooled trunk features of up to ``capacity`` frames, float32 [capacity, F] on the model's
    device."""

    def __init__(self, model, capacity: int, half=False):
        if half:
            raise RuntimeError("FramePool: fp32 only (a 16-bit trunk's features are not the ones a "
                               "density was fitted on)")
        capacity = int(capacity)
        if not 1 <= capacity <= 1 << 24:
            raise ValueError("capacity must be in 1..2^24")
        self.model = model
        self.F = int(model.FEATURES)
        self.device = next(model.parameters()).device
        self.capacity = capacity
        self.pool = torch.empty(capacity, self.F, dtype=torch.float32, device=self.device)
        self.count = 0
        self.weights_key = 0

    def __len__(self):
        return self.count

    def features(self):
        """View [count, F] of the rows added so far."""
        return self.pool[:self.count]

    def clear(self):
        self.count, self.weights_key = 0, 0

    # ---- filling ---------------------------------------------------------------------------------
    def _room(self, b, who):
        if self.count + b > self.capacity:
            raise RuntimeError(f"FramePool.{who}: the pool is full ({self.count} + {b} rows, "
                               f"capacity {self.capacity})")
        return self.pool[self.count:self.count + b]

    def add_features(self, features):
        """The op-level form: append rows of already pooled features (float32 [B, ld >= F], features
        first).  A device copy; no synchronise."""
        if features.dim() != 2 or features.dtype != torch.float32 or features.size(1) < self.F:
            raise RuntimeError(f"FramePool.add_features: features must be float32 [B, >= {self.F}], "
                               f"got {features.dtype} {tuple(features.shape)}")
        b = features.size(0)
        self._room(b, "add_features").copy_(features[:, :self.F])
        self.count += b
        return self

    def add(self, images, speeds, commands):
        """One batch of the log: the module's fp32 eval-mode forward (as FeatureDensity.update runs
        it), then a device copy of the pooled features it left into the next rows of the pool.
        Nothing is copied to the host.  Keep the model in eval mode between two adds: anything that
        may have changed the weights (a train() / eval() switch included) raises."""
        if self.device.type != "cuda":
            raise RuntimeError("FramePool.add needs the model on an MI355X (no CPU fallback)")
        self._room(images.size(0), "add")
        eng = self.model.engine()
        if eng.train_precision != "fp32":
            raise RuntimeError("FramePool.add: fp32 only (the engine is set to 16-bit plans)")
        was_training = self.model.training
        self.model.eval()
        with torch.no_grad():
            self.model(images, speeds, commands)
        key = int(eng.weights_key())
        if was_training:
            self.model.train()
        if self.weights_key and key != self.weights_key:
            raise RuntimeError("FramePool.add: the weights changed since the first add; clear() "
                               "starts a new pool")
        self.weights_key = key
        return self.add_features(eng.plan_features(eng.last_plan))

    # ---- the launches (host tests replace them) ------------------------------------------------------
    def _need_device(self, who):
        if self.device.type != "cuda":
            raise RuntimeError(f"FramePool.{who} needs the pool on an MI355X (no CPU fallback)")

    def _cover_op(self, rows, centres, mind):
        """cilrs_kcenter_cover: mind = min(mind, distance to every centre)"""
        self._need_device("select")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_kcenter_cover(
            L.ptr(rows), rows.stride(0), rows.size(0), rows.size(1), L.ptr(centres),
            centres.stride(0), centres.size(0), L.ptr(mind), L.C.c_void_p(stream)))

    def _greedy_op(self, rows, mind, k):
        """cilrs_kcenter_greedy: k picks; returns (sel int64 [k], radius float32 [k]) on the device"""
        self._need_device("select")
        n = rows.size(0)
        sel = torch.empty(k, dtype=torch.int64, device=rows.device)
        radius = torch.empty(k, dtype=torch.float32, device=rows.device)
        nbytes = L.lib().cilrs_kcenter_scratch_bytes(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=rows.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_kcenter_greedy(
            L.ptr(rows), rows.stride(0), n, rows.size(1), L.ptr(mind), k, L.ptr(sel), L.ptr(radius),
            L.ptr(scratch), nbytes, L.C.c_void_p(stream)))
        return sel, radius

    def _kmeans_scratch(self, rows, k):
        nbytes = L.lib().cilrs_kmeans_scratch_bytes(rows.size(0), rows.size(1), k)
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=rows.device), nbytes

    def _assign_op(self, rows, centres, labels, dist, counts, inertia, changed):
        """cilrs_kmeans_assign: labels int32 [N] (in: the labels `changed` is counted against), dist
        float32 [N], counts int64 [K], inertia float64 [1], changed int64 [1]"""
        self._need_device("cluster")
        scratch, nbytes = self._kmeans_scratch(rows, centres.size(0))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_kmeans_assign(
            L.ptr(rows), rows.stride(0), rows.size(0), rows.size(1), L.ptr(centres), centres.stride(0),
            centres.size(0), L.ptr(labels), L.ptr(dist), L.ptr(counts), L.ptr(inertia), L.ptr(changed),
            L.ptr(scratch), nbytes, L.C.c_void_p(stream)))

    def _update_op(self, rows, labels, centres, counts):
        """cilrs_kmeans_update: centres [K, F] become the means of their rows; counts int64 [K]"""
        self._need_device("cluster")
        scratch, nbytes = self._kmeans_scratch(rows, centres.size(0))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_kmeans_update(
            L.ptr(rows), rows.stride(0), rows.size(0), rows.size(1), L.ptr(labels), L.ptr(centres),
            centres.stride(0), centres.size(0), L.ptr(counts), L.ptr(scratch), nbytes,
            L.C.c_void_p(stream)))

    def _lloyd_op(self, rows, centres, iters, labels, dist, counts, inertia, changed):
        """cilrs_kmeans_lloyd: `iters` times (assign, update) and a closing assign, in place;
        inertia float64 / changed int64 [iters + 1]"""
        self._need_device("cluster")
        scratch, nbytes = self._kmeans_scratch(rows, centres.size(0))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_kmeans_lloyd(
            L.ptr(rows), rows.stride(0), rows.size(0), rows.size(1), L.ptr(centres), centres.stride(0),
            centres.size(0), iters, L.ptr(labels), L.ptr(dist), L.ptr(counts), L.ptr(inertia),
            L.ptr(changed), L.ptr(scratch), nbytes, L.C.c_void_p(stream)))

    # ---- nearest neighbours (cilrs_mi355.neighbours) -----------------------------------------------
    index_class = None                    # host tests put a NeighbourIndex with replaced launches here

    def index(self, density=None):
        """A NeighbourIndex over a copy of the rows added so far.  density: a finalised
        FeatureDensity -- the rows are whitened through cilrs_feature_whiten (Mahalanobis metric)
        and the index keeps the tables that whiten a query the same way.  None: Euclidean."""
        from .neighbours import NeighbourIndex
        cls = self.index_class or NeighbourIndex
        if self.count == 0:
            raise RuntimeError("FramePool.index: the pool is empty")
        if density is None:
            return cls(self.features().clone(), weights_key=self.weights_key)
        density._need_finalized("index")
        if density.F != self.F:
            raise RuntimeError(f"FramePool.index: the density was fitted on {density.F} features, "
                               f"the pool holds {self.F}")
        return cls(self.features(), "mahalanobis", density._origin().clone(), density.W.clone(),
                   weights_key=density.fit_weights_key or self.weights_key, commands=density.NC,
                   whitened=False)

    def _check_index(self, index, who):
        """an index of ANOTHER set whose rows the pool's features can be compared with"""
        if index.F != self.F:
            raise RuntimeError(f"FramePool.{who}: the index holds {index.F} features, the pool "
                               f"{self.F}")
        if index.device != self.device:
            raise RuntimeError(f"FramePool.{who}: the index is on {index.device}, the pool on "
                               f"{self.device}")
        if self.count == 0:
            raise RuntimeError(f"FramePool.{who}: the pool is empty")

    def nearest(self, index, k=1):
        """The k rows of ``index`` (a NeighbourIndex of another set, e.g. everything labelled so far)
        nearest to every row of the pool, in the index's metric: ``index.join(pool.features(), k)``,
        (idx int64 [count, k], dist float32 [count, k]) on the device."""
        self._check_index(index, "nearest")
        return index.join(self.features(), k)

    def novel_rows(self, index, radius2):
        """The pool rows whose nearest row of ``index`` is farther than the squared distance
        ``radius2``, int64 ascending on the device: what a drive adds to the labelled set."""
        _idx, dist = self.nearest(index, 1)
        return (dist[:, 0] > float(radius2)).nonzero().reshape(-1)

    # ---- selection -------------------------------------------------------------------------------
    @staticmethod
    def _kernel_rows(t):
        """float32 rows as the kernels take them: unit column stride, 16-byte aligned rows"""
        if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            t = t.contiguous()
        return t

    def select(self, k, density=None, covered=None, first=None, covered_index=None) -> Selection:
        """Greedy k-center over the rows added so far: up to ``k`` picks, each the row farthest from
        everything covered before it.

        density   a finalised FeatureDensity: the rows are ``density.whiten(pool)`` (Mahalanobis
                  metric) and the fit's command means count as covered.  None: the raw features,
                  Euclidean.
        covered   float32 [M, >= F] of frames already labelled or chosen earlier; covered as well.
        first     with nothing to cover, the row that is the first centre (default row 0).
        covered_index  a NeighbourIndex of the labelled set, of any size, in the metric of this
                  call; its rows count as covered, through ``NeighbourIndex.join``'s kernels.
                  The index's rows are compared with this call's rows as they are: with rows
                  ``density.whiten(C)`` (``whitened=True``) the picks and radii are those of
                  ``covered=C`` bit for bit; ``index(density)`` of another pool whitens through
                  cilrs_feature_whiten, whose rounding differs from ``density.whiten``'s in the
                  last bits."""
        n, k = self.count, int(k)
        if n == 0:
            raise RuntimeError("FramePool.select: the pool is empty")
        if not 1 <= k <= n:
            raise ValueError(f"k must be in 1..{n} (the rows in the pool)")
        if self.F % 4 or not 4 <= self.F <= 2048:
            raise RuntimeError(f"FramePool.select: feature width {self.F}")
        rows, centres, metric = self.features(), [], "euclidean"
        if density is not None:
            density._need_finalized("whiten")
            if density.F != self.F:
                raise RuntimeError(f"FramePool.select: the density was fitted on {density.F} "
                                   f"features, the pool holds {self.F}")
            rows, metric = density.whiten(rows), "mahalanobis"
            centres.append(density.whitened_means())
        if covered is not None:
            if covered.dim() != 2 or covered.dtype != torch.float32 or covered.size(1) < self.F or \
                    covered.size(0) > 65536:
                raise RuntimeError(f"FramePool.select: covered must be float32 [M <= 65536, >= "
                                   f"{self.F}], got {covered.dtype} {tuple(covered.shape)}")
            covered = covered.to(rows.device)
            if covered.size(0):
                centres.append(density.whiten(covered) if density is not None
                               else covered[:, :self.F])
        if first is not None:
            if centres:
                raise ValueError("first: only with nothing to cover (no density, no covered rows)")
            first = int(first)
            if not 0 <= first < n:
                raise ValueError(f"first must be in 0..{n - 1}")
            centres.append(rows[first:first + 1])
        if covered_index is not None:
            if first is not None:
                raise ValueError("first: only with nothing to cover (no covered_index)")
            self._check_index(covered_index, "select")
            want = "euclidean" if density is None else "mahalanobis"
            if covered_index.metric != want:
                raise RuntimeError(f"FramePool.select: covered_index is {covered_index.metric}, this "
                                   f"selection {want}")
            if density is not None and not (torch.equal(covered_index.origin, density._origin().to(
                    covered_index.device)) and torch.equal(covered_index.W, density.W.to(covered_index.device))):
                raise RuntimeError("FramePool.select: covered_index was whitened with other tables than "
                                   "`density`")
        rows = self._kernel_rows(rows)
        mind = torch.full((n,), float("inf"), dtype=torch.float32, device=rows.device)
        for c in centres:
            self._cover_op(rows, self._kernel_rows(c), mind)
        if covered_index is not None:
            d = covered_index._join_whitened(rows, 1)[1][:, 0]     # rows: this call's coordinates
            mind = torch.where(d < mind, d, mind)
        picks = k if first is None else k - 1
        if picks:
            sel, radius = self._greedy_op(rows, mind, picks)
        else:
            sel = torch.empty(0, dtype=torch.int64, device=rows.device)
            radius = torch.empty(0, dtype=torch.float32, device=rows.device)
        if rows.device.type == "cuda":
            torch.cuda.current_stream(rows.device).synchronize()
        sel, radius = sel.cpu().numpy(), radius.cpu().numpy()
        if first is not None:
            sel = np.concatenate([np.array([first], dtype=np.int64), sel])
            radius = np.concatenate([np.array([np.inf], dtype=np.float32), radius])
        zero = np.flatnonzero(radius == 0.0)
        if zero.size:
            sel, radius = sel[:zero[0]], radius[:zero[0]]
        return Selection(sel, radius, mind, metric, rows)

    # ---- clustering (cilrs_mi355.cluster) --------------------------------------------------------
    def cluster(self, k, density=None, iters=50, init="kcenter", check_every=5):
        """K-means over the rows added so far (include/cilrs_hip.h "K-means"): a Clustering with
        centres, a label and a squared distance per row, the cluster sizes and the histories.

        density      a finalised FeatureDensity: the Mahalanobis metric of ``select`` (the rows go
                     through cilrs_feature_whiten, the kernel that whitens every later query).
                     None: the raw features, Euclidean.
        init         "kcenter": the picks of ``select(k, density=density)`` (raises when the pool holds
                     fewer than k distinct rows); int64 row indices [k]; or float32 centres
                     [k, >= F] of raw features, whitened first when a density is given.
        iters        at most this many (assign, update) iterations, then a closing assign.
        check_every  iterations per cilrs_kmeans_lloyd call: one synchronise per block, and the run
                     stops at the first block that holds an assignment with no change."""
        from .cluster import cluster
        return cluster(self, k, density, iters, init, check_every)
