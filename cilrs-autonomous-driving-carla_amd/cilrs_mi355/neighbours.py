"""Which recorded frames does this tick look like to the trunk?  The k nearest rows of a FramePool.

``saliency``, ``attribution`` and ``gradcam`` explain a tick through pixels, ``predict_novelty`` gives
one number under a Gaussian assumption.  This module answers with examples: the k pool rows nearest
to a feature vector, defined in include/cilrs_hip.h ("Nearest neighbours") and computed by one
streaming pass over the pool per eight queries (csrc/knn.hip), or for many queries at once by a
matrix-core screen with an exact re-score and a per-query certificate (csrc/knn_join.hip, "Bulk
nearest neighbours"; what it cannot certify goes through the streaming pass).  The distance to the
k-th neighbour is the non-parametric novelty score of Sun et al. (2022); the same query
de-duplicates new frames against a labelled set and picks the labelled frames that sit next to a new
one in a fine-tuning batch.

    index = pool.index(density=fd)                      # Mahalanobis; pool.index() is Euclidean
    idx, dist = index.query(pool.features()[:4], k=8)   # device tensors, no synchronise
    index.calibrate(k=8)                                # leave-one-out over the index's own rows
    idx, dist = index.join(drive_features, k=8)         # query() for a whole drive: the same bits, k <= 16,
    idx, dist = index.graph(k=8)                        #   and for the index's own rows (leave-one-out)
    controls, pred_speed, idx, dist = predictor.predict_neighbours(frames, kmh, commands, index, k=8)
    if index.percentile(dist[0, -1]) > 99.0: ...        # a threshold with a meaning

With a density the pool's rows and every query go through ONE whitening kernel
(cilrs_feature_whiten), so a pool row queried against its own index is at distance exactly 0.
fp32 only.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

METRICS = ("euclidean", "mahalanobis")
WHITEN_CHUNK = 4096       # rows per cilrs_feature_whiten call (its scratch is chunk * F floats)
QUERY_CHUNK = 4096        # queries per cilrs_knn call of calibrate()
MAX_K = 64
JOIN_MAX_K = 16           # cilrs_knn_join keeps K + 8 <= 24 candidates per lane in LDS
JOIN_CHUNK = 65536        # queries per cilrs_knn_join call
JOIN_MIN_Q = 64           # below this many queries join() is query(): the measured crossover at 176,256 x 512
                          # (profiles/knn_join_bench.log; 32 queries for k = 1, 64 for k = 8 and 16)


class NeighbourIndex:
    """The rows of a pool on the device -- float32 [N, F], whitened when the metric is
    ``"mahalanobis"`` -- with the tables that whiten a query (``origin`` [F], ``W`` [F, F]) and the
    ``weights_key`` of the weights the pool's features came from."""

    def __init__(self, rows, metric="euclidean", origin=None, W=None, weights_key=0, commands=0,
                 whitened=True, capacity: int = 1 << 12):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}")
        if (metric == "mahalanobis") != (origin is not None and W is not None):
            raise ValueError("origin and W go with the mahalanobis metric, and only with it")
        if rows.dim() != 2 or rows.dtype != torch.float32 or rows.size(0) < 1:
            raise RuntimeError(f"NeighbourIndex: rows must be float32 [N >= 1, F], got {rows.dtype} "
                               f"{tuple(rows.shape)}")
        self.metric = metric
        self.F = int(rows.size(1))
        self.device = rows.device
        self.weights_key = int(weights_key)
        self.commands = int(commands)         # of the density's fit (0: none)
        self.origin = None if origin is None else origin.to(self.device, torch.float32).contiguous()
        self.W = None if W is None else W.to(self.device, torch.float32).contiguous()
        if self.W is not None and (tuple(self.W.shape) != (self.F, self.F) or
                                   tuple(self.origin.shape) != (self.F,)):
            raise RuntimeError(f"NeighbourIndex: origin / W do not fit {self.F} features")
        if self.F % 4 or not 4 <= self.F <= 2048:
            raise RuntimeError(f"NeighbourIndex: feature width {self.F}")
        if not rows.size(0) <= 1 << 24:
            raise RuntimeError("NeighbourIndex: more than 2^24 rows")
        self.rows = rows.contiguous() if whitened or self.W is None else self.whiten(rows)
        self._capacity = int(capacity)
        self.log, self.log_count, self.log_k, self._sorted = None, 0, 0, None
        self.last_join = None                 # {"queries", "uncertified"} of the last join / graph

    def __len__(self):
        return int(self.rows.size(0))

    # ---- the launches (host tests replace them) ------------------------------------------------------
    def _need_device(self, who):
        if self.device.type != "cuda":
            raise RuntimeError(f"NeighbourIndex.{who} needs the index on an MI355X (no CPU fallback)")

    def _whiten_op(self, features, y):
        """cilrs_feature_whiten: y [B, F] = tril(W) (features[:, :F] - origin)"""
        self._need_device("whiten")
        if self.F not in (512, 2048):
            raise RuntimeError(f"NeighbourIndex.whiten: feature width {self.F} (512 or 2048)")
        b = features.size(0)
        n = L.lib().cilrs_feature_whiten_scratch_floats(self.F, b)
        scratch = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_feature_whiten(
            L.ptr(features), features.stride(0), b, self.F, L.ptr(self.origin), L.ptr(self.W),
            L.ptr(y), L.ptr(scratch), n, L.C.c_void_p(stream)))

    def _knn_op(self, queries, k, skip, idx, dist):
        """cilrs_knn of queries [Q, ld >= F] against the rows into idx int64 / dist float32 [Q, k]"""
        self._need_device("query")
        n, q = self.rows.size(0), queries.size(0)
        nbytes = L.lib().cilrs_knn_scratch_bytes(n, q, k)
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_knn(
            L.ptr(self.rows), self.rows.stride(0), n, self.F, L.ptr(queries), queries.stride(0), q,
            L.ptr(skip), k, L.ptr(idx), L.ptr(dist), L.ptr(scratch), nbytes, L.C.c_void_p(stream)))

    def _join_op(self, queries, k, skip, idx, dist, uncertified, n_uncertified):
        """cilrs_knn_join of queries [Q <= 65536, ld >= F] against the rows: idx / dist as _knn_op for
        the certified queries, -2 / NaN and uncertified[q] = 1 (int32 [Q], their count in int32 [1])
        for the others"""
        self._need_device("join")
        n, q = self.rows.size(0), queries.size(0)
        nbytes = L.lib().cilrs_knn_join_scratch_bytes(n, q, self.F, k)
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_knn_join(
            L.ptr(self.rows), self.rows.stride(0), n, self.F, L.ptr(queries), queries.stride(0), q,
            L.ptr(skip), k, L.ptr(idx), L.ptr(dist), L.ptr(uncertified), L.ptr(n_uncertified),
            L.ptr(scratch), nbytes, L.C.c_void_p(stream)))

    # ---- queries ---------------------------------------------------------------------------------
    def _check_features(self, features, who):
        if features.dim() == 1:
            features = features[None]
        if features.dim() != 2 or features.dtype != torch.float32 or features.size(1) < self.F:
            raise RuntimeError(f"NeighbourIndex.{who}: features must be float32 [Q, >= {self.F}], got "
                               f"{features.dtype} {tuple(features.shape)}")
        features = features.to(self.device)
        if features.stride(1) != 1 or features.stride(0) % 4 or features.data_ptr() % 16:
            features = features[:, :self.F].contiguous()
        return features

    def _check_k(self, k):
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}")
        return k

    def whiten(self, features):
        """Raw features [B, >= F] in the coordinates of the index's rows: float32 [B, F].  The
        Euclidean metric has none of its own: the first F columns come back."""
        features = self._check_features(features, "whiten")
        if self.W is None:
            return features[:, :self.F]
        y = torch.empty(features.size(0), self.F, dtype=torch.float32, device=self.device)
        for b0 in range(0, features.size(0), WHITEN_CHUNK):
            self._whiten_op(features[b0:b0 + WHITEN_CHUNK], y[b0:b0 + WHITEN_CHUNK])
        return y

    def _query_rows(self, queries, k, skip):
        """queries already in the rows' coordinates"""
        q = queries.size(0)
        idx = torch.empty(q, k, dtype=torch.int64, device=self.device)
        dist = torch.empty(q, k, dtype=torch.float32, device=self.device)
        if skip is not None:
            skip = torch.as_tensor(skip, dtype=torch.int64).reshape(-1).to(self.device).contiguous()
            if skip.numel() != q:
                raise RuntimeError(f"NeighbourIndex.query: skip must hold one row index per query "
                                   f"({q}), got {skip.numel()}")
        for q0 in range(0, q, 65536):
            self._knn_op(queries[q0:q0 + 65536], k, None if skip is None else skip[q0:q0 + 65536],
                         idx[q0:q0 + 65536], dist[q0:q0 + 65536])
        return idx, dist

    def query(self, features, k, skip=None):
        """The k rows nearest to each raw feature vector: (idx int64 [Q, k], dist float32 [Q, k]) on
        the device, ascending in (dist, idx), squared distances; no synchronise.  ``skip`` [Q]: a
        row each query must not return (leave-one-out for queries that are pool rows).  With fewer
        than k candidates the last slots hold -1 / +inf."""
        k = self._check_k(k)
        features = self._check_features(features, "query")
        if features.size(0) == 0:
            return (torch.empty(0, k, dtype=torch.int64, device=self.device),
                    torch.empty(0, k, dtype=torch.float32, device=self.device))
        return self._query_rows(self.whiten(features) if self.W is not None else features, k, skip)

    def _check_join_k(self, k, who):
        k = int(k)
        if not 1 <= k <= JOIN_MAX_K:
            raise ValueError(f"NeighbourIndex.{who}: k must be in 1..{JOIN_MAX_K}; NeighbourIndex.query "
                             f"takes k up to {MAX_K}")
        return k

    def _join_rows(self, queries, k, skip):
        """_query_rows through the matrix-core screen: cilrs_knn_join per 65,536 queries, then the
        queries it could not certify through cilrs_knn.  Bit for bit _query_rows' result.  One
        synchronise per chunk (the count of flagged queries is read on the host).  Returns
        (idx, dist, flagged queries)."""
        q = queries.size(0)
        idx = torch.empty(q, k, dtype=torch.int64, device=self.device)
        dist = torch.empty(q, k, dtype=torch.float32, device=self.device)
        if skip is not None:
            skip = torch.as_tensor(skip, dtype=torch.int64).reshape(-1).to(self.device).contiguous()
            if skip.numel() != q:
                raise RuntimeError(f"NeighbourIndex.join: skip must hold one row index per query "
                                   f"({q}), got {skip.numel()}")
        flagged = 0
        for q0 in range(0, q, JOIN_CHUNK):
            y = queries[q0:q0 + JOIN_CHUNK]
            sk = None if skip is None else skip[q0:q0 + JOIN_CHUNK]
            unc = torch.empty(y.size(0), dtype=torch.int32, device=self.device)
            n_unc = torch.empty(1, dtype=torch.int32, device=self.device)
            self._join_op(y, k, sk, idx[q0:q0 + JOIN_CHUNK], dist[q0:q0 + JOIN_CHUNK], unc, n_unc)
            n = int(n_unc.item())
            if n:
                at = unc.nonzero().reshape(-1)
                i2, d2 = self._query_rows(y.index_select(0, at), k,
                                          None if sk is None else sk.index_select(0, at))
                idx[q0:q0 + JOIN_CHUNK].index_copy_(0, at, i2)
                dist[q0:q0 + JOIN_CHUNK].index_copy_(0, at, d2)
                flagged += n
        return idx, dist, flagged

    def join(self, features, k, skip=None):
        """``query`` for a whole drive: the same contract and the same bits with k <= 16, computed by
        the matrix-core screen of cilrs_knn_join (include/cilrs_hip.h "Bulk nearest neighbours") and,
        for the queries the screen cannot certify, by ``query``'s own kernel.  Synchronises once per
        65,536 queries.  ``last_join`` = {"queries": Q, "uncertified": queries that fell back}.
        Below JOIN_MIN_Q queries it is ``query``."""
        k = self._check_join_k(k, "join")
        features = self._check_features(features, "join")
        return self._join_whitened(self.whiten(features) if self.W is not None else features, k, skip)

    def _join_whitened(self, queries, k, skip=None):
        """join of queries already in the rows' coordinates (FramePool.select has them)"""
        q = queries.size(0)
        if q < JOIN_MIN_Q:
            self.last_join = {"queries": q, "uncertified": 0}
            return self._query_rows(queries, k, skip)
        idx, dist, flagged = self._join_rows(queries, k, skip)
        self.last_join = {"queries": q, "uncertified": flagged}
        return idx, dist

    def graph(self, k):
        """The k nearest other rows of every row of the index (the leave-one-out self-join):
        ``query(rows, k, skip=arange(N))`` bit for bit, through ``join``'s kernels on views of the
        rows."""
        k = self._check_join_k(k, "graph")
        n = len(self)
        idx = torch.empty(n, k, dtype=torch.int64, device=self.device)
        dist = torch.empty(n, k, dtype=torch.float32, device=self.device)
        flagged = 0
        for q0 in range(0, n, JOIN_CHUNK):
            q1 = min(n, q0 + JOIN_CHUNK)
            i2, d2, f = self._join_rows(self.rows[q0:q1], k, torch.arange(q0, q1, dtype=torch.int64))
            idx[q0:q1], dist[q0:q1] = i2, d2
            flagged += f
        self.last_join = {"queries": n, "uncertified": flagged}
        return idx, dist

    def score(self, features, k):
        """The squared distance to the k-th nearest row, float32 [Q] on the device."""
        return self.query(features, k)[1][:, self._check_k(k) - 1]

    # ---- calibration --------------------------------------------------------------------------
    def _log_room(self, b):
        if self.log is None:
            self.log = torch.empty(max(self._capacity, b), dtype=torch.float32, device=self.device)
        if self.log_count + b > self.log.numel():
            grown = torch.empty(max(2 * self.log.numel(), self.log_count + b), dtype=torch.float32,
                                device=self.device)
            grown[:self.log_count] = self.log[:self.log_count]
            self.log = grown
        return self.log[self.log_count:self.log_count + b]

    def calibrate(self, k, rows=None, bulk=False):
        """Leave-one-out k-th neighbour distances of the index's own rows -- all, or the subset
        ``rows`` (int64 indices) -- into a device log; ``quantile`` / ``percentile`` read from it.
        Every call with another k starts the log again.  ``bulk``: through ``join``'s kernels
        (k <= 16, one synchronise per 65,536 rows): the same log bit for bit."""
        k = self._check_join_k(k, "calibrate(bulk=True)") if bulk else self._check_k(k)
        n = len(self)
        if rows is None:
            rows = torch.arange(n, dtype=torch.int64)
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
            raise ValueError(f"rows must be in 0..{n - 1}")
        if k != self.log_k:
            self.log_count, self.log_k, self._sorted = 0, k, None
        rows = rows.to(self.device)
        chunk = JOIN_CHUNK if bulk else QUERY_CHUNK
        for q0 in range(0, rows.numel(), chunk):
            r = rows[q0:q0 + chunk]
            if bulk:
                dist = self._join_rows(self.rows.index_select(0, r), k, r)[1]
            else:
                dist = self._query_rows(self.rows.index_select(0, r), k, r)[1]
            self._log_room(r.numel()).copy_(dist[:, k - 1])
            self.log_count += r.numel()
            self._sorted = None
        return self

    def calibration_scores(self):
        """The sorted calibration scores, float32 on the host (one copy per change of the log)."""
        if self._sorted is None:
            if self.log_count == 0:
                raise RuntimeError("NeighbourIndex: no calibration scores; call calibrate() first")
            self._sorted = np.sort(self.log[:self.log_count].cpu().numpy())
        return self._sorted

    def quantile(self, q):
        """The k-th neighbour distance below which a fraction ``q`` (0..1) of the rows fell."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must be in [0, 1]")
        return float(np.quantile(self.calibration_scores().astype(np.float64), q))

    def percentile(self, d2):
        """Share (0..100) of the calibration rows whose score was <= ``d2``; scalar or array."""
        s = self.calibration_scores()
        r = 100.0 * np.searchsorted(s, np.asarray(d2, dtype=np.float32), side="right") / s.size
        return float(r) if np.ndim(r) == 0 else r

    # ---- what a predictor checks ------------------------------------------------------------------
    def check_model(self, model, who="query"):
        """Raise when this index does not describe ``model``'s features."""
        f = int(model.FEATURES)
        if f != self.F:
            raise RuntimeError(f"NeighbourIndex.{who}: the index holds {self.F} features, the model "
                               f"has {f}")
        if self.commands and int(model.num_commands) != self.commands:
            raise RuntimeError(f"NeighbourIndex.{who}: the density was fitted for {self.commands} "
                               f"commands, the model has {int(model.num_commands)}")

    # ---- persistence --------------------------------------------------------------------------
    def state_dict(self):
        """Plain tensors and numbers (loadable under ``weights_only``)."""
        def cpu(t):
            return None if t is None else t.detach().cpu().clone()
        cal = torch.from_numpy(self.calibration_scores().copy()) if self.log_count else \
            torch.empty(0, dtype=torch.float32)
        return {"F": self.F, "N": len(self), "metric": self.metric, "weights_key": self.weights_key,
                "commands": self.commands, "rows": cpu(self.rows), "origin": cpu(self.origin),
                "W": cpu(self.W), "calibration": cal, "calibration_k": int(self.log_k)}

    def load_state_dict(self, sd):
        if int(sd["F"]) != self.F:
            raise RuntimeError(f"NeighbourIndex.load_state_dict: saved with {int(sd['F'])} features, "
                               f"this index has {self.F}")
        dev = self.device
        self.metric = str(sd["metric"])
        self.weights_key, self.commands = int(sd["weights_key"]), int(sd["commands"])
        self.rows = sd["rows"].to(device=dev, dtype=torch.float32).contiguous()
        self.origin = None if sd["origin"] is None else sd["origin"].to(dev, torch.float32).contiguous()
        self.W = None if sd["W"] is None else sd["W"].to(dev, torch.float32).contiguous()
        self.log, self.log_count, self._sorted = None, 0, None
        self.log_k = int(sd["calibration_k"])
        cal = sd["calibration"]
        if cal.numel():
            self._log_room(cal.numel()).copy_(cal.to(torch.float32))
            self.log_count = cal.numel()
        return self

    def save(self, path):
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path, device="cpu"):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        index = cls(sd["rows"].to(device), sd["metric"], sd["origin"], sd["W"])
        return index.load_state_dict(sd)
