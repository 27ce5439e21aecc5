"""What does a recorded drive consist of, and how much of each kind?  K-means over a FramePool.

``FeatureDensity`` scores one frame, ``FramePool.select`` picks the extremes worth labelling,
``FramePool.index`` finds the recorded frames a tick resembles.  This module partitions the pool into
scenario modes: Lloyd's iteration as defined in include/cilrs_hip.h ("K-means"), deterministic and
bit-identical from run to run, seven launches per iteration and no host round trip inside a block of
iterations (csrc/kmeans.hip).  The reference balances its sampler by command only
(``data.class_balanced_weights``); ``balanced_weights`` is the cluster counterpart.

    c = pool.cluster(64, density=fd, iters=50)          # Mahalanobis; farthest-point seeding
    c.sizes, c.medoids()                                # rows per mode, a representative frame each
    idx = data.weighted_indices(c.balanced_weights(), num_samples)
    c.histogram(other_pool.features())                  # a later drive under the same centres
    labels, dist = c.assign(features)                   # bit for bit the Lloyd assignment
    predictor.predict_neighbours(frames, kmh, commands, c.index(), k=1)     # a tick's cluster id

With a density the pool's rows, float32 initial centres and every later query go through ONE
whitening kernel (cilrs_feature_whiten, as ``FramePool.index`` does), so ``assign`` of a pool row
returns that row's label and distance exactly.  fp32 only.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from .neighbours import METRICS, NeighbourIndex

MAX_K = 1024
MAX_ITERS = 10000


class Clustering:
    """centres float32 [K, F] (device; whitened when the metric is ``"mahalanobis"``), labels int32
    [N] and dist float32 [N] (device; squared distances, -1 / +inf for a row with no candidate), sizes
    int64 [K], the inertia / changed histories (one entry per assignment) on the host, and the
    tables that whiten a later query (``origin`` [F], ``W`` [F, F]).  rows: the device rows the
    clustering ran on (not saved)."""

    index_class = None                    # host tests put a NeighbourIndex with replaced launches here

    def __init__(self, centres, labels, dist, sizes, inertia, changed, iterations, converged,
                 metric="euclidean", origin=None, W=None, weights_key=0, commands=0, rows=None,
                 index_class=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}")
        if centres.dim() != 2 or centres.dtype != torch.float32:
            raise RuntimeError(f"Clustering: centres must be float32 [K, F], got {centres.dtype} "
                               f"{tuple(centres.shape)}")
        self.centres = centres.contiguous()
        self.K, self.F = int(centres.size(0)), int(centres.size(1))
        self.device = centres.device
        self.labels, self.dist = labels, dist
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.inertia = np.asarray(inertia, dtype=np.float64)
        self.changed = np.asarray(changed, dtype=np.int64)
        self.iterations, self.converged = int(iterations), bool(converged)
        self.metric = metric
        self.origin, self.W = origin, W
        self.weights_key, self.commands = int(weights_key), int(commands)
        self.rows = rows
        if index_class is not None:
            self.index_class = index_class
        self._index = None

    def __len__(self):
        return self.K

    # ---- later features --------------------------------------------------------------------------
    def index(self):
        """A NeighbourIndex over the centres, with the tables that whiten a query:
        ``predict_neighbours(..., index=c.index(), k=1)`` returns a tick's cluster id."""
        if self._index is None:
            cls = self.index_class or NeighbourIndex
            self._index = cls(self.centres, self.metric, self.origin, self.W,
                              weights_key=self.weights_key, commands=self.commands, whitened=True)
        return self._index

    def assign(self, features):
        """(labels int32 [Q], dist float32 [Q]) of raw features [Q, >= F] on the device, no
        synchronise: cilrs_knn over the centres with k = 1, by definition bit for bit the Lloyd
        assignment."""
        idx, dist = self.index().query(features, 1)
        return idx[:, 0].to(torch.int32), dist[:, 0].contiguous()

    def histogram(self, features):
        """Rows per cluster of another drive's features, int64 [K] on the host (rows with no
        candidate are not counted)."""
        labels = self.assign(features)[0].cpu().numpy()
        return np.bincount(labels[labels >= 0], minlength=self.K).astype(np.int64)

    def medoids(self, rows=None):
        """int64 [K] on the host: the pool row nearest each centre (cilrs_knn with X = the rows the
        clustering ran on, Y = the centres, K = 1).  rows: those rows again, for a loaded
        clustering."""
        rows = self.rows if rows is None else rows
        if rows is None:
            raise RuntimeError("Clustering.medoids: a loaded clustering does not hold the pool's rows; "
                               "pass them (whitened as the centres are)")
        cls = self.index_class or NeighbourIndex
        idx, _dist = cls(rows, whitened=True)._query_rows(self.centres, 1, None)
        return idx[:, 0].cpu().numpy()

    def balanced_weights(self):
        """float64 [N] on the host, N / (K' sizes[label]) with K' the non-empty clusters (0 for a row
        with no label): every non-empty cluster carries the same total weight.  The cluster
        counterpart of ``data.class_balanced_weights``, ready for ``data.weighted_indices``."""
        labels = self.labels.cpu().numpy()
        live = int((self.sizes > 0).sum())
        w = len(labels) / (max(live, 1) * np.where(self.sizes > 0, self.sizes, 1).astype(np.float64))
        return np.where(labels >= 0, w[np.maximum(labels, 0)], 0.0)

    # ---- persistence --------------------------------------------------------------------------
    def state_dict(self):
        """Plain tensors and numbers (loadable under ``weights_only``)."""
        def cpu(t):
            return None if t is None else t.detach().cpu().clone()
        return {"F": self.F, "K": self.K, "metric": self.metric, "weights_key": self.weights_key,
                "commands": self.commands, "centres": cpu(self.centres), "labels": cpu(self.labels),
                "dist": cpu(self.dist), "sizes": torch.from_numpy(self.sizes.copy()),
                "inertia": torch.from_numpy(self.inertia.copy()),
                "changed": torch.from_numpy(self.changed.copy()), "iterations": self.iterations,
                "converged": self.converged, "origin": cpu(self.origin), "W": cpu(self.W)}

    def load_state_dict(self, sd):
        if int(sd["F"]) != self.F:
            raise RuntimeError(f"Clustering.load_state_dict: saved with {int(sd['F'])} features, this "
                               f"clustering has {self.F}")
        dev = self.device

        def there(t, dtype):
            return None if t is None else t.to(device=dev, dtype=dtype).contiguous()
        self.metric = str(sd["metric"])
        self.weights_key, self.commands = int(sd["weights_key"]), int(sd["commands"])
        self.centres = there(sd["centres"], torch.float32)
        self.K = int(self.centres.size(0))
        self.labels, self.dist = there(sd["labels"], torch.int32), there(sd["dist"], torch.float32)
        self.sizes = sd["sizes"].numpy().astype(np.int64)
        self.inertia = sd["inertia"].numpy().astype(np.float64)
        self.changed = sd["changed"].numpy().astype(np.int64)
        self.iterations, self.converged = int(sd["iterations"]), bool(sd["converged"])
        self.origin, self.W = there(sd["origin"], torch.float32), there(sd["W"], torch.float32)
        self.rows, self._index = None, None
        return self

    def save(self, path):
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path, device="cpu"):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        c = cls(sd["centres"].to(device), None, None, sd["sizes"].numpy(), [], [], 0, False,
                sd["metric"])
        return c.load_state_dict(sd)


def cluster(pool, k, density=None, iters=50, init="kcenter", check_every=5) -> Clustering:
    """FramePool.cluster (see there)."""
    n = pool.count
    if n == 0:
        raise RuntimeError("FramePool.cluster: the pool is empty")
    k, iters, check_every = int(k), int(iters), int(check_every)
    if not 1 <= k <= min(n, MAX_K):
        raise ValueError(f"k must be in 1..{min(n, MAX_K)} (the rows in the pool, at most {MAX_K})")
    if not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"iters must be in 0..{MAX_ITERS}")
    if check_every < 1:
        raise ValueError("check_every must be at least 1")
    F = pool.F
    if F % 4 or not 4 <= F <= 2048:
        raise RuntimeError(f"FramePool.cluster: feature width {F}")
    if isinstance(init, str) and init != "kcenter":
        raise ValueError(f"init must be 'kcenter', int64 row indices [{k}] or float32 centres "
                         f"[{k}, >= {F}], got {init!r}")
    index_cls = pool.index_class or NeighbourIndex
    origin = W = None
    metric, weights_key, commands = "euclidean", pool.weights_key, 0
    rows = pool.features()
    whiten = lambda t: t[:, :F]
    if density is not None:
        density._need_finalized("whiten")
        if density.F != F:
            raise RuntimeError(f"FramePool.cluster: the density was fitted on {density.F} features, "
                               f"the pool holds {F}")
        metric, origin, W = "mahalanobis", density._origin().clone(), density.W.clone()
        weights_key, commands = density.fit_weights_key or pool.weights_key, density.NC
        # the whitening every later query goes through: one kernel, a row's result depends on the row alone
        white = index_cls(rows[:1], metric, origin, W, whitened=True)
        whiten = white.whiten
        origin, W = white.origin, white.W

    # ---- seeding -----------------------------------------------------------------------------
    picks = None
    if isinstance(init, str):
        s = pool.select(k, density=density)
        if len(s.indices) < k:
            raise RuntimeError(f"FramePool.cluster: the pool holds {len(s.indices)} distinct rows under "
                               f"this metric, fewer than k = {k}")
        picks = torch.from_numpy(s.indices)
    else:
        init = torch.as_tensor(init)
        if init.dtype == torch.int64 and init.dim() == 1:
            if init.numel() != k or int(init.min()) < 0 or int(init.max()) >= n:
                raise ValueError(f"init: {k} row indices in 0..{n - 1}")
            picks = init
        elif init.dtype == torch.float32 and init.dim() == 2:
            if init.size(0) != k or init.size(1) < F:
                raise ValueError(f"init: float32 centres [{k}, >= {F}], got {tuple(init.shape)}")
        else:
            raise ValueError(f"init must be 'kcenter', int64 row indices [{k}] or float32 centres "
                             f"[{k}, >= {F}], got {init.dtype} {tuple(init.shape)}")
    rows = pool._kernel_rows(whiten(rows) if density is not None else rows)
    if picks is not None:
        centres = rows.index_select(0, picks.to(rows.device))[:, :F].contiguous()
    else:
        centres = whiten(init.to(rows.device)).contiguous().clone()

    # ---- Lloyd in blocks of check_every iterations, one synchronise per block -----------------------
    dev = rows.device
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros(k, dtype=torch.int64, device=dev)
    inertia, changed = [], []
    done, converged = 0, False
    while True:
        block = min(check_every, iters - done)
        ine = torch.zeros(block + 1, dtype=torch.float64, device=dev)
        chg = torch.zeros(block + 1, dtype=torch.int64, device=dev)
        pool._lloyd_op(rows, centres, block, labels, dist, counts, ine, chg)
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()
        ine, chg = ine.cpu().numpy(), chg.cpu().numpy()
        # a block's first assignment repeats the closing one of the block before it
        first = 0 if not inertia else 1
        inertia.extend(ine[first:].tolist())
        changed.extend(chg[first:].tolist())
        done += block
        converged = bool((chg[first:] == 0).any()) if (first or block) else False
        if converged or done >= iters:
            break
    if converged:                                            # iterations up to the first fixed point
        done = int(np.flatnonzero(np.asarray(changed) == 0)[0])
    return Clustering(centres, labels, dist, counts.cpu().numpy(), inertia, changed, done, converged,
                      metric, origin, W, weights_key, commands, rows=rows, index_class=pool.index_class)
