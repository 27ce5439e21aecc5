"""K nearest neighbours in float64: the definition of include/cilrs_hip.h ("Nearest neighbours")
restated with numpy, a brute-force form of it, and what the device tests derive their expected
results from (test_knn_host.py, test_knn_gpu.py)."""
import numpy as np

import _kcenter as KC


def order(d, K, skip=-1):
    """(idx int64 [K], dist [K]) of one query from its distances d [N]: the K candidates smallest in
    (d, i), ascending; row i is no candidate when i == skip or d[i] is NaN; empty slots -1 / +inf.
    The dtype of d is kept, so a device's own fp32 distances give the device's expected result."""
    d = np.asarray(d)
    i = np.arange(len(d), dtype=np.int64)
    cand = ~np.isnan(d) & (i != int(skip))
    i, v = i[cand], d[cand]
    o = np.lexsort((i, v))[:K]                               # the last key is the primary one
    idx = np.full(K, -1, dtype=np.int64)
    dist = np.full(K, np.inf, dtype=d.dtype)
    idx[:len(o)], dist[:len(o)] = i[o], v[o]
    return idx, dist


def knn(X, Y, K, skip=None):
    """(idx int64 [Q][K], dist float64 [Q][K]) of the definition, d in float64 of the fp32 values"""
    Y = np.asarray(Y, dtype=np.float32).reshape(-1, np.asarray(X).shape[1])
    idx = np.empty((len(Y), K), dtype=np.int64)
    dist = np.empty((len(Y), K))
    for q, y in enumerate(Y):
        with np.errstate(invalid="ignore", over="ignore"):
            d = KC.dist(X, y)
        idx[q], dist[q] = order(d, K, -1 if skip is None else skip[q])
    return idx, dist


def brute(X, Y, K, skip=None):
    """the same by sorting Python tuples: no numpy ordering involved"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out_i, out_d = [], []
    for q, y in enumerate(Y):
        pairs = []
        for i, x in enumerate(X):
            d = float(sum((a - b) * (a - b) for a, b in zip(x, y)))
            if d != d or (skip is not None and int(skip[q]) == i):
                continue
            pairs.append((d, i))
        pairs.sort()
        pairs = pairs[:K] + [(float("inf"), -1)] * (K - len(pairs[:K]))
        out_i.append([p[1] for p in pairs])
        out_d.append([p[0] for p in pairs])
    return np.array(out_i, dtype=np.int64), np.array(out_d)


def whiten64(v, origin, W):
    """tril(W) (fp32(v - origin)) in float64 of the fp32 tables, and sum_j |W_ij||u_j| per entry"""
    u = (np.asarray(v, dtype=np.float32) - np.asarray(origin, dtype=np.float32)[None, :]).astype(np.float64)
    W = np.tril(np.asarray(W, dtype=np.float32).astype(np.float64))
    return u @ W.T, np.abs(u) @ np.abs(W).T
