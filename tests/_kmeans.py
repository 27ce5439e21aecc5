"""K-means in float64: the definition of include/cilrs_hip.h ("K-means") restated with numpy, a
brute-force pure-Python form of it, planted blobs, and the checker the device tests go through
(test_kmeans_host.py, test_kmeans_gpu.py).

The checker walks the DEVICE'S OWN sequence of (centres, labels), as _kcenter.check_greedy walks the
device's picks, so a near-tie between two centres cannot make a test flaky.  With b = KC.bound(D):

  labels     (1 - 2b) d64(X_i, C[label_i]) <= min_m d64(X_i, C_m): the device compares fp32 distances,
             each within b of its float64 value, so its winner is within (1 + b) / (1 - b) < 1 / (1 - 2b)
             of the float64 minimum.  -1 only where every float64 distance is NaN.
  dist       within b relative of d64.
  counts     exact, from the device's labels; changed exact.
  centres    the fp32 rounding of the float64 mean over the device's labels, to at most one fp32 ulp:
             the order of a float64 sum of n terms moves it by at most n 2^-53 relative, which can
             cross an fp32 rounding boundary and cannot do more.  On integer-valued rows every sum is
             exact: bit for bit.  Empty clusters unchanged, bit for bit.
  inertia    within N 2^-53 relative of math.fsum of the device's own dist (N - 1 float64 additions
             of non-negative terms, each half an ulp).
  monotone   J64[t + 1] <= (1 + 3b) J64[t] + s, J64 the float64 objective of the device's centres and
             labels: for fixed labels the exact mean mu minimises the objective and a centre
             mu + e costs n_m |e|^2 more, |e_j| <= 2^-24 |C_mj| for the rounded mean (the first term
             of s = sum_m n_m sum_j (2^-24 |C_mj|)^2); the next assignment then takes, row by row, a
             centre within 1 / (1 - 2b) < 1 + 3b of the best one, which is no farther than the row's
             previous centre.
"""
import math

import numpy as np

import _kcenter as KC


def dist_matrix(X, C):
    """float64 [N][K] of d(X_i, C_m) on the fp32 values"""
    X = np.asarray(X, dtype=np.float32)
    C = np.asarray(C, dtype=np.float32).reshape(-1, X.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([KC.dist(X, c) for c in C], axis=1)


def assign(X, C):
    """(label int32 [N], dist float64 [N]): the smallest in (d, m), NaN distances no candidates, -1 /
    +inf with none"""
    d = dist_matrix(X, C)
    cand = ~np.isnan(d)
    key = np.where(cand, d, np.inf)
    label = np.argmin(key, axis=1).astype(np.int32)          # the first of equal values
    # a row whose candidates are all +inf: argmin of the key may sit on a NaN before them
    for i in np.flatnonzero(~cand[np.arange(len(label)), label]):
        c = np.flatnonzero(cand[i])
        label[i] = c[0] if c.size else -1
    best = np.where(label >= 0, d[np.arange(len(label)), np.maximum(label, 0)], np.inf)
    return label, best


def counts(label, K):
    label = np.asarray(label)
    return np.bincount(label[(label >= 0) & (label < K)], minlength=K).astype(np.int64)


def means(X, label, C):
    """float64 [K][D]: the mean of the rows of each label; a cluster with no rows keeps C's row"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    out = np.asarray(C, dtype=np.float32).astype(np.float64).copy()
    for m in range(len(out)):
        rows = X64[np.asarray(label) == m]
        if len(rows):
            out[m] = np.array([math.fsum(col) for col in rows.T]) / len(rows)
    return out


def update(X, label, C):
    """the centres after an update, fp32"""
    return means(X, label, C).astype(np.float32)


def lloyd(X, C, iters, label=None):
    """(C fp32, label, dist float64, counts, inertia [iters + 1], changed [iters + 1])"""
    X = np.asarray(X, dtype=np.float32)
    C = np.array(C, dtype=np.float32)
    label = np.full(len(X), -1, dtype=np.int32) if label is None else np.asarray(label, dtype=np.int32)
    inertia, changed = [], []
    for t in range(iters + 1):
        new, d = assign(X, C)
        changed.append(int((new != label).sum()))
        inertia.append(math.fsum(d[new >= 0]))
        label = new
        if t < iters:
            C = update(X, label, C)
    return C, label, d, counts(label, len(C)), np.array(inertia), np.array(changed, dtype=np.int64)


def brute_lloyd(X, C, iters):
    """the same with Python floats and lists: no numpy ordering or reduction involved"""
    X = [[float(v) for v in row] for row in np.asarray(X, dtype=np.float32)]
    C = [[float(v) for v in row] for row in np.asarray(C, dtype=np.float32)]
    label = [-1] * len(X)
    for t in range(iters + 1):
        for i, x in enumerate(X):
            best, arg = float("inf"), -1
            for m, c in enumerate(C):
                d = math.fsum((a - b) * (a - b) for a, b in zip(x, c))
                if d != d:
                    continue
                if arg < 0 or d < best:
                    best, arg = d, m
            label[i] = arg
        if t < iters:
            for m in range(len(C)):
                rows = [x for x, l in zip(X, label) if l == m]
                if rows:
                    C[m] = [float(np.float32(math.fsum(col) / len(rows))) for col in zip(*rows)]
    return np.array(C, dtype=np.float32), np.array(label, dtype=np.int32)


def objective(X, C, label):
    """J64: the float64 objective of these centres and labels (rows labelled -1 take no part)"""
    label = np.asarray(label)
    d = dist_matrix(X, C)
    on = label >= 0
    return math.fsum(d[np.flatnonzero(on), label[on]])


def rounding_slack(C, n):
    """s = sum_m n_m sum_j (2^-24 |C_mj|)^2"""
    C64 = np.asarray(C, dtype=np.float32).astype(np.float64)
    return float((np.asarray(n, dtype=np.float64) * ((2.0 ** -24 * np.abs(C64)) ** 2).sum(axis=1)).sum())


def check_assign(X, C, label_before, label, dist, cnt, inertia, changed, what="assign"):
    """one assignment of the device against the definition; returns the largest share of the
    distance bound used"""
    X = np.asarray(X, dtype=np.float32)
    N, D = X.shape
    K = len(C)
    b = KC.bound(D)
    label = np.asarray(label)
    got = np.asarray(dist, dtype=np.float32)
    assert label.dtype == np.int32 and label.shape == (N,) and got.shape == (N,), what
    assert ((label >= -1) & (label < K)).all(), (what, label.min(), label.max())
    d = dist_matrix(X, C)
    none = np.isnan(d).all(axis=1)
    assert np.array_equal(label < 0, none), f"{what}: -1 exactly where every float64 distance is NaN"
    assert (got[none] == np.inf).all(), f"{what}: dist of a row with no candidate is not +inf"
    on = np.flatnonzero(~none)
    mine = d[on, label[on]]
    assert not np.isnan(mine).any(), f"{what}: a label whose distance is NaN"
    low = np.nanmin(d[on], axis=1)
    bad = (1.0 - 2.0 * b) * mine > low
    assert not bad.any(), (what, on[bad][:8], label[on][bad][:8], mine[bad][:8], low[bad][:8])
    ok = KC.close(got[on], mine, b)
    assert ok.all(), (what, on[~ok][:8], got[on][~ok][:8], mine[~ok][:8])
    assert np.array_equal(np.asarray(cnt), counts(label, K)), (what, cnt)
    assert int(changed) == int((label != np.asarray(label_before)).sum()), (what, changed)
    want = math.fsum(float(v) for v in got[on])
    assert abs(float(inertia) - want) <= N * 2.0 ** -53 * want, (what, inertia, want)
    fin = np.isfinite(mine) & (mine > 0)
    return float((np.abs(got[on][fin] - mine[fin]) / (b * mine[fin])).max()) if fin.any() else 0.0


def check_update(X, label, C_before, C_after, exact=False, what="update"):
    """the centres after the device's update against the float64 means over the given labels;
    returns the share of centre entries that differ from the rounded mean (by one ulp)"""
    before = np.asarray(C_before, dtype=np.float32)
    got = np.asarray(C_after, dtype=np.float32)
    K = len(before)
    n = counts(label, K)
    want = means(X, label, before).astype(np.float32)
    empty = n == 0
    assert np.array_equal(got[empty].view(np.uint32), before[empty].view(np.uint32)), \
        f"{what}: an empty cluster's centre changed"
    if exact:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: not bit for bit"
        return 0.0
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), what
    return float((got != want).mean())


def check_steps(X, C0, label0, steps, what="lloyd"):
    """steps: per assignment t the device's (C_t, label, dist, counts, inertia, changed), C_t the
    centres the assignment ran on -- C_0 = C0, C_{t + 1} the update of C_t under label_t.  Checks every
    assignment, every update and the monotone objective; returns the J64 history."""
    D = np.asarray(X).shape[1]
    b = KC.bound(D)
    J = []
    prev_label, prev_C = np.asarray(label0), np.asarray(C0, dtype=np.float32)
    for t, (C, label, dist, cnt, inertia, changed) in enumerate(steps):
        C = np.asarray(C, dtype=np.float32)
        if t == 0:
            assert np.array_equal(C.view(np.uint32), prev_C.view(np.uint32)), what
        else:
            check_update(X, prev_label, prev_C, C, what=f"{what}: update {t - 1}")
        check_assign(X, C, prev_label, label, dist, cnt, inertia, changed, f"{what}: assign {t}")
        J.append(objective(X, C, label))
        if t:
            s = rounding_slack(C, counts(prev_label, len(C)))
            assert J[t] <= (1.0 + 3.0 * b) * J[t - 1] + s, (what, t, J[t - 1], J[t], s)
        prev_label, prev_C = np.asarray(label), C
    return np.array(J)


def blobs(K, per, D, seed, sep=8.0):
    """Planted blobs (K <= D): relu rows of scale 1 / sqrt(D) -- a row's norm is about 0.7, a blob's
    diameter about 1 -- plus an offset of norm `sep` in the blob's own block of D // K coordinates,
    so two blobs are sep * sqrt(2) apart.  Returns (X fp32 [K * per][D] shuffled, truth [N]);
    blob_geometry measures what was planted."""
    assert K <= D
    rng = np.random.default_rng(seed)
    base = KC.relu_rows(K * per, D, seed, scale=1.0 / np.sqrt(D))
    truth = np.repeat(np.arange(K), per)
    off = np.zeros((K, D), dtype=np.float32)
    w = D // K
    for m in range(K):
        off[m, m * w:(m + 1) * w] = sep / np.sqrt(w)
    X = base + off[truth]
    order = rng.permutation(len(X))
    return X[order].astype(np.float32), truth[order]


def blob_geometry(X, truth):
    """(largest blob diameter, smallest distance between rows of different blobs), Euclidean"""
    X64 = np.asarray(X, dtype=np.float64)
    g = np.sqrt(np.maximum(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1), 0.0))
    same = truth[:, None] == truth[None, :]
    return float(g[same].max()), float(g[~same].min())


def same_partition(label, truth):
    """label equals truth up to a permutation of the cluster ids"""
    label, truth = np.asarray(label), np.asarray(truth)
    pairs = set(zip(label.tolist(), truth.tolist()))
    return len(pairs) == len(set(truth.tolist())) == len({p[0] for p in pairs}) and (label >= 0).all()
