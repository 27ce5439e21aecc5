"""Bulk k-NN on the host: the float64 must-certify predicate of tests/_knn_join.py against a
brute-force count, and the Python around cilrs_knn_join -- NeighbourIndex.join / graph /
calibrate(bulk=True), FramePool.nearest / novel_rows / select(covered_index=) -- with the launches
replaced by numpy stand-ins: the routing below JOIN_MIN_Q, the gather and scatter of the queries the
entry flags, the chunks of 65,536 queries with skip, the refusals and the log.

The stand-in of cilrs_knn_join answers like the entry (idx / dist of the definition, -2 / NaN and a
flag for the queries a rule picks, their count); which queries it flags is the test's choice, the
result of join must not depend on it."""
import numpy as np
import pytest
import torch

import _kcenter as KC
import _knn as KN
import _knn_join as KJ
import test_kcenter_host as TK
import test_novelty_host as TH
from cilrs_mi355 import NeighbourIndex
from cilrs_mi355 import neighbours as NB


# ---- the predicate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(12, 4, 1), (30, 4, 2), (30, 8, 3), (9, 4, 1), (40, 12, 16)])
def test_must_certify_against_a_brute_force_count(N, D, K):
    assert KJ.candidates(K) == K + 8 and KJ.candidates(KJ.MAX_K) == 24
    assert KJ.bound(D) == KC.bound(D) and KJ.c_D(D) == 2 * D + 16
    hits = 0
    for seed in range(6):
        X = KC.relu_rows(N, D, seed)
        Y = np.concatenate([KC.relu_rows(6, D, 50 + seed), X[:3], X[:2] + 30.0])
        if seed % 2:
            X[N // 2:] += 3000.0                   # large norms: E_q eats the gaps between the near rows
        for skip in (None, np.array([-1, 0, 1, N, 2, 3, 0, 1, 2, 0, 1])):
            a, b = KJ.must_certify(X, Y, K, skip), KJ.must_certify_brute(X, Y, K, skip)
            assert np.array_equal(a, b), (seed, a, b)
            hits += int(a.sum())
    print(f"N={N} D={D} K={K}: the predicate holds for {hits} of {6 * 2 * 11}")
    if N <= KJ.candidates(K):
        assert hits == 6 * 2 * 11                  # every row is a candidate
    elif N // 2 > KJ.candidates(K):
        assert 0 < hits < 6 * 2 * 11               # the cases decide both ways
    # nothing has to be certified once a norm is not finite
    X = KC.relu_rows(40, 4, 1)
    Y = KC.relu_rows(5, 4, 2)
    Y[2, 0] = np.nan
    assert not KJ.must_certify(X, Y, 1)[2]
    X[3, 1] = 3e19
    assert not KJ.must_certify(X, Y, 1).any()
    assert abs(KJ.screen_error(512, 3.0, 1.0) - 1040 * 4.0 * 2.0 ** -24) < 1e-18


# ---- stand-ins ----------------------------------------------------------------------------------------
def _host_knn(X, Y, k, skip):
    """the definition (tests/_knn.py) for many queries at once: (idx int64, dist float32) [Q][k]"""
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((Y64[:, None, :] - X64[None, :, :]) ** 2).sum(-1).astype(np.float32)
    Q, N = d.shape
    out = np.isnan(d)
    if skip is not None:
        s = np.asarray(skip, dtype=np.int64)
        ok = (s >= 0) & (s < N)
        out[np.flatnonzero(ok), s[ok]] = True
    rows = np.broadcast_to(np.arange(N), (Q, N))
    order = np.lexsort((rows, np.where(out, np.float32(np.inf), d), out), axis=-1)[:, :k]
    idx = np.full((Q, k), -1, dtype=np.int64)
    dist = np.full((Q, k), np.inf, dtype=np.float32)
    n = min(k, N)
    keep = ~np.take_along_axis(out, order, axis=1)
    idx[:, :n] = np.where(keep, order, -1)
    dist[:, :n] = np.where(keep, np.take_along_axis(d, order, axis=1), np.float32(np.inf))
    return idx, dist


class _HostJoinIndex(NeighbourIndex):
    """launches replaced; `flag(query rows of the call) -> bool mask` picks what the entry flags"""
    flag = staticmethod(lambda y: np.zeros(len(y), dtype=bool))

    def _whiten_op(self, features, y):
        z, _ = KN.whiten64(features[:, :self.F].numpy(), self.origin.numpy(), self.W.numpy())
        y.copy_(torch.from_numpy(z.astype(np.float32)))

    def _knn_op(self, queries, k, skip, idx, dist):
        self.calls.append(("knn", queries.size(0)))
        i, d = _host_knn(self.rows.numpy(), queries[:, :self.F].numpy(), k, None if skip is None else skip.numpy())
        idx.copy_(torch.from_numpy(i))
        dist.copy_(torch.from_numpy(d))

    def _join_op(self, queries, k, skip, idx, dist, uncertified, n_uncertified):
        assert 1 <= queries.size(0) <= 65536 and 1 <= k <= 16 and queries.stride(1) == 1
        assert uncertified.dtype == n_uncertified.dtype == torch.int32 and n_uncertified.numel() == 1
        assert skip is None or (skip.dtype == torch.int64 and skip.numel() == queries.size(0))
        self.calls.append(("join", queries.size(0)))
        y = queries[:, :self.F].numpy()
        i, d = _host_knn(self.rows.numpy(), y, k, None if skip is None else skip.numpy())
        f = np.asarray(self.flag(y), dtype=bool)
        i[f], d[f] = -2, np.nan
        idx.copy_(torch.from_numpy(i))
        dist.copy_(torch.from_numpy(d))
        uncertified.copy_(torch.from_numpy(f.astype(np.int32)))
        n_uncertified.fill_(int(f.sum()))


def _index(X, flag=None, **kw):
    ix = _HostJoinIndex(torch.from_numpy(np.ascontiguousarray(X)), **kw)
    ix.calls = []
    if flag is not None:
        ix.flag = flag
    return ix


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- join ---------------------------------------------------------------------------------------------
def test_join_routes_small_calls_to_query_and_scatters_what_the_entry_flags():
    F, N, k = 8, 50, 5
    X = KC.relu_rows(N, F, 1)
    first_col_large = lambda y: y[:, 0] > 0.5              # noqa: E731
    ix = _index(X, first_col_large)
    for Q, joined in ((NB.JOIN_MIN_Q - 1, False), (NB.JOIN_MIN_Q, True), (NB.JOIN_MIN_Q + 77, True)):
        Y = torch.from_numpy(KC.relu_rows(Q, F + 4, 2 + Q))   # wider than F: the first F columns count
        flagged = int(first_col_large(Y.numpy()).sum())
        assert 0 < flagged < Q
        for skip in (None, torch.arange(Q) % (N + 3)):
            ix.calls = []
            got = ix.join(Y, k, skip=skip)
            assert ix.last_join == {"queries": Q, "uncertified": flagged if joined else 0}
            assert ix.calls == ([("join", Q), ("knn", flagged)] if joined else [("knn", Q)])
            want = ix.query(Y, k, skip=skip)
            assert _same(got, want)
            assert bool((got[0] >= -1).all()) and not bool(torch.isnan(got[1]).any())
            if skip is not None:
                assert not bool((got[0] == skip[:, None]).any())
    # nothing flagged: no second launch; everything flagged: all of them, in order
    ix.flag = _HostJoinIndex.flag
    ix.calls = []
    Y = torch.from_numpy(KC.relu_rows(200, F, 9))
    assert _same(ix.join(Y, k), ix.query(Y, k)) and ix.calls[:1] == [("join", 200)] and ("knn", 200) == ix.calls[1]
    assert len(ix.calls) == 2                                  # the join, then query()'s own launch
    ix.flag = lambda y: np.ones(len(y), dtype=bool)
    ix.calls = []
    got = ix.join(Y, k)
    assert ix.calls == [("join", 200), ("knn", 200)] and ix.last_join["uncertified"] == 200
    assert _same(got, ix.query(Y, k))
    assert tuple(ix.join(Y[:0], 3)[0].shape) == (0, 3)
    for bad in (0, 17, 64):
        with pytest.raises(ValueError, match="query"):
            ix.join(Y, bad)
    with pytest.raises(RuntimeError, match="one row index per query"):
        ix.join(Y, k, skip=torch.arange(5))
    with pytest.raises(RuntimeError, match="features must be"):
        ix.join(Y[:, :4], k)


def test_join_chunks_above_65536_queries_with_skip():
    F, N, k = 4, 20, 3
    X = KC.relu_rows(N, F, 3)
    Q = 65536 + 300
    Y = torch.from_numpy(KC.relu_rows(Q, F, 4))
    every_seventh = lambda y: (np.round(y[:, 1] * 1000).astype(np.int64) % 7) == 0     # noqa: E731
    ix = _index(X, every_seventh)
    skip = torch.arange(Q) % (N + 2)
    got = ix.join(Y, k, skip=skip)
    f = every_seventh(Y.numpy())
    assert ix.calls == [("join", 65536), ("knn", int(f[:65536].sum())), ("join", 300), ("knn", int(f[65536:].sum()))]
    assert ix.last_join == {"queries": Q, "uncertified": int(f.sum())}
    i, d = _host_knn(X, Y.numpy(), k, skip.numpy())
    assert np.array_equal(got[0].numpy(), i) and np.array_equal(got[1].numpy().view(np.uint32), d.view(np.uint32))
    assert not bool((got[0] == skip[:, None]).any())


def test_graph_and_bulk_calibration():
    pool, fd, vt, rows = _pools()
    for index in (pool.index(), pool.index(density=fd)):
        index.calls = []
        index.flag = lambda y: y[:, 0] > np.median(y[:, 0])
        k = 4
        gi, gd = index.graph(k)
        want = index.query(index.rows, k, skip=torch.arange(rows)) if index.W is None else \
            index._query_rows(index.rows, k, torch.arange(rows))
        assert _same((gi, gd), want) and not bool((gi == torch.arange(rows)[:, None]).any())
        assert index.last_join["queries"] == rows and 0 < index.last_join["uncertified"] < rows
        index.calibrate(k)
        slow = index.log[:index.log_count].clone()
        index.calibrate(k + 1)
        index.calls = []
        index.calibrate(k, bulk=True)
        assert index.calls[0] == ("join", rows) and index.log_count == rows
        assert torch.equal(index.log[:rows].view(torch.int32), slow.view(torch.int32))
        index.calibrate(k, rows=[3, 1], bulk=True)
        assert index.log_count == rows + 2 and torch.equal(index.log[rows:rows + 2], gd[[3, 1], k - 1])
        assert index.percentile(np.inf) == 100.0
        with pytest.raises(ValueError, match="1..16"):
            index.calibrate(17, bulk=True)
        with pytest.raises(ValueError, match="1..16"):
            index.graph(0)


# ---- FramePool ----------------------------------------------------------------------------------------
class _HostPool(TK._HostPool):
    index_class = _HostJoinIndex


def _pools():
    fd, vt, _ct, rows = TH._fitted()
    fd.finalize()
    pool = _HostPool(TH._Stub(), capacity=rows)
    pool.add_features(vt[:rows])

    class _Calls(_HostJoinIndex):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls = []
    pool.index_class = _Calls
    return pool, fd, vt, rows


def test_nearest_novel_rows_and_select_with_a_covered_index():
    pool, fd, vt, rows = _pools()
    F = pool.F
    assert rows >= NB.JOIN_MIN_Q, "the pool of the host fixtures is at least one query tile"
    labelled = vt[:60, :F].clone() + 0.25
    labelled[:10] = vt[5:15, :F]                               # ten labelled frames are in the drive
    lab_pool = _HostPool(TH._Stub(), capacity=60)
    lab_pool.index_class = pool.index_class
    lab_pool.add_features(labelled)
    ix = lab_pool.index()
    ix.flag = lambda y: y[:, 1] > np.median(y[:, 1])
    idx, dist = pool.nearest(ix, 2)
    assert _same((idx, dist), ix.query(pool.features(), 2)) and ix.calls[0] == ("join", rows)
    assert torch.equal(idx[5:15, 0], torch.arange(10)) and not dist[5:15, 0].any()
    d1 = dist[:, 0].numpy()
    r2 = np.float32(np.sort(d1)[rows // 2])
    assert np.array_equal(pool.novel_rows(ix, r2).numpy(), np.flatnonzero(d1 > r2))
    assert len(pool.novel_rows(ix, np.inf)) == 0 and 5 not in pool.novel_rows(ix, 0.0).tolist()
    # select: the index's rows count as covered exactly as covered= counts them
    k = 6
    a = pool.select(k, covered=labelled)
    b = pool.select(k, covered_index=ix)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.radius, b.radius)
    assert torch.equal(a.min_dist, b.min_dist) and ix.last_join["queries"] == rows
    # ... with a density: rows whitened as the selection whitens them, after the command means
    wix = pool.index_class(fd.whiten(labelled).contiguous(), "mahalanobis", fd._origin().clone(), fd.W.clone())
    wix.flag = ix.flag
    a = pool.select(k, density=fd, covered=labelled)
    b = pool.select(k, density=fd, covered_index=wix)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.radius, b.radius) and len(b.indices) == k
    assert b.metric == "mahalanobis"
    # refusals
    with pytest.raises(RuntimeError, match="euclidean"):
        pool.select(k, density=fd, covered_index=ix)
    with pytest.raises(RuntimeError, match="mahalanobis"):
        pool.select(k, covered_index=wix)
    moved = pool.index_class(wix.rows, "mahalanobis", fd._origin().clone() + 1.0, fd.W.clone())
    with pytest.raises(RuntimeError, match="other tables"):
        pool.select(k, density=fd, covered_index=moved)
    with pytest.raises(ValueError, match="first"):
        pool.select(k, first=2, covered_index=ix)
    narrow = pool.index_class(torch.zeros(5, F - 4))
    for call in (lambda: pool.nearest(narrow), lambda: pool.select(k, covered_index=narrow)):
        with pytest.raises(RuntimeError, match="features"):
            call()
    with pytest.raises(ValueError, match="query"):
        pool.nearest(ix, 17)
    with pytest.raises(RuntimeError, match="empty"):
        _HostPool(TH._Stub(), capacity=4).nearest(ix)
