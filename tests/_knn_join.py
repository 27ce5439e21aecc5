"""The guarantees of the matrix-core screen of include/cilrs_hip.h ("Bulk nearest neighbours")
restated in float64 with numpy: K_s, b, E_q and the must-certify predicate the device tests hold
cilrs_knn_join to (test_knn_join_gpu.py, test_knn_join_host.py)."""
import numpy as np

import _kcenter as KC

MAX_K = 16
U = 2.0 ** -24


def candidates(K):
    """K_s of the header: K + 8"""
    return K + 8


def bound(D):
    """b: the relative error of one fp32 distance (tests/_kcenter.py)"""
    return KC.bound(D)


def c_D(D):
    return 2 * D + 16


def norms(X):
    """float64 sums of squares of the fp32 rows"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.einsum("ij,ij->i", X, X)


def screen_error(D, nx_max, ny):
    """E_q = c_D 2^-24 (max_i nx_i + ny_q)"""
    return c_D(D) * U * (nx_max + ny)


def eligible(d64, skip):
    """rows that are candidates of the definition: not the skipped one, no NaN distance"""
    ok = ~np.isnan(d64)
    if skip is not None and 0 <= int(skip) < len(d64):
        ok[int(skip)] = False
    return ok


def must_certify(X, Y, K, skip=None):
    """bool [Q]: the queries cilrs_knn_join has to certify.  With finite rows and queries whose
    norms stay far from overflow, q must be certified when no more than K_s rows are eligible (every
    one is then a candidate), or when
        d64_(K) (1 + b) < (1 - b) (d64_(K_s) - 2 E_q),
    d64_(j) the j-th smallest float64 distance among the eligible rows: the K nearest rows then
    precede every row beyond the K_s-th in s as well (each s + ny is within E of its distance), the
    K-th fp32 result is at most (1 + b) d64_(K), and sigma + ny is at least d64_(K_s) - E.  Queries
    for which this returns False may or may not be certified."""
    X = np.asarray(X, dtype=np.float32)
    Y = np.asarray(Y, dtype=np.float32)
    N, D = X.shape
    Ks, b = candidates(K), bound(D)
    nx = norms(X)
    out = np.zeros(len(Y), dtype=bool)
    if not np.isfinite(nx).all() or nx.max() >= 2.0 ** 120:
        return out
    ny = norms(Y)
    for q, y in enumerate(Y):
        if not np.isfinite(ny[q]) or ny[q] >= 2.0 ** 120:
            continue
        d = KC.dist(X, y)
        ok = eligible(d, None if skip is None else skip[q])
        d = np.sort(d[ok])
        if len(d) <= Ks:
            out[q] = True
        elif len(d) >= K:
            E = screen_error(D, nx.max(), ny[q])
            out[q] = d[K - 1] * (1.0 + b) < (1.0 - b) * (d[Ks - 1] - 2.0 * E)
    return out


def must_certify_brute(X, Y, K, skip=None):
    """the same predicate without sorting: counts instead of order statistics (tiny inputs only)"""
    X = np.asarray(X, dtype=np.float32)
    Y = np.asarray(Y, dtype=np.float32)
    N, D = X.shape
    Ks, b = candidates(K), bound(D)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    out = np.zeros(len(Y), dtype=bool)
    for q in range(len(Y)):
        ds = []
        nxs = []
        for i in range(N):
            nxs.append(float(sum(v * v for v in X64[i])))
            if skip is not None and int(skip[q]) == i:
                continue
            ds.append(float(sum((X64[i][j] - Y64[q][j]) ** 2 for j in range(D))))
        ny = float(sum(v * v for v in Y64[q]))
        if len(ds) <= Ks:
            out[q] = True
            continue
        E = c_D(D) * U * (max(nxs) + ny)
        # the j-th smallest: the smallest value with at least j values <= it
        def kth(j):
            return min(v for v in ds if sum(1 for w in ds if w <= v) >= j)
        out[q] = kth(K) * (1.0 + b) < (1.0 - b) * (kth(Ks) - 2.0 * E)
    return out
