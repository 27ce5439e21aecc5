"""K-means on the host: the float64 definition (tests/_kmeans.py) against a brute-force pure-Python
Lloyd, its NaN and tie rules, the planted blobs the device tests reuse, and
cilrs_mi355.FramePool.cluster / Clustering with the launches replaced by the definition.

Planted blobs.  With a separation s between rows of different blobs above twice the largest blob
diameter d (blob_geometry measures both), farthest-point selection takes one row per blob: while a
blob has no pick, its rows are at least s from every pick and every row of a picked blob is at most
d < s from one, so the next pick falls in an unpicked blob.  Every row is then within d of its own
blob's seed and at least s > 2 d from any other, the first assignment is the planted partition, a
centre is a mean of its blob's rows and stays within d of each of them, and nothing changes again.
"""
import numpy as np
import pytest
import torch

import _kcenter as KC
import _kmeans as KM
import test_knn_host as TKH
import test_novelty_host as TH
from cilrs_mi355 import Clustering, FramePool
from cilrs_mi355 import data as DATA

F0 = TH.F0


# ---- the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,seed", [(7, 4, 1, 0), (12, 4, 3, 1), (30, 8, 4, 2), (25, 12, 5, 3)])
def test_definition_against_a_brute_force_lloyd(n, d, k, seed):
    X = KC.relu_rows(n, d, seed) + np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    C0 = X[:k].copy()
    for iters in (0, 1, 4):
        C, label, dist, cnt, inertia, changed = KM.lloyd(X, C0, iters)
        Cb, lb = KM.brute_lloyd(X, C0, iters)
        assert np.array_equal(label, lb) and np.array_equal(C.view(np.uint32), Cb.view(np.uint32))
        assert len(inertia) == len(changed) == iters + 1 and changed[0] == n and cnt.sum() == n
        assert np.array_equal(cnt, KM.counts(label, k))
        assert (np.diff(inertia) <= 1e-12 * inertia[:-1]).all()
        assert abs(inertia[-1] - KM.objective(X, C, label)) <= 1e-12 * inertia[-1]
        steps = []
        Ct, lt = C0, np.full(n, -1, dtype=np.int32)
        for t in range(iters + 1):                           # the definition passes its own checker
            new, dt = KM.assign(X, Ct)
            steps.append((Ct, new, dt.astype(np.float32), KM.counts(new, k),
                          float(np.sum(dt.astype(np.float32).astype(np.float64))), int((new != lt).sum())))
            Ct, lt = KM.update(X, new, Ct), new
        KM.check_steps(X, C0, np.full(n, -1, dtype=np.int32), steps)
    # iters1 then iters2 from the labels and centres reached is iters1 + iters2
    C1, l1, *_ = KM.lloyd(X, C0, 2)
    C2, l2, _d, _c, _i, ch2 = KM.lloyd(X, C1, 2, l1)
    assert np.array_equal(C2.view(np.uint32), C.view(np.uint32)) and np.array_equal(l2, label) and ch2[0] == 0


def test_nan_and_tie_rules():
    X = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [np.nan, 0, 0, 0], [3e19, 0, 0, 0], [1, 0, 0, 0]], dtype=np.float32)
    Cn = np.array([[np.nan, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    label, dist = KM.assign(X, Cn)
    assert label.tolist() == [2, 1, -1, 1, 1]                # duplicates and the tie of row 4: the lowest index
    assert dist[0] == 0 and dist[1] == 0 and dist[2] == np.inf and dist[4] == 1
    assert KM.counts(label, 5).tolist() == [0, 3, 1, 0, 0]
    new = KM.update(X, label, Cn)
    assert np.isnan(new[0, 0]) and np.array_equal(new[3], Cn[3]) and np.array_equal(new[4], Cn[4])   # empty: kept
    assert np.array_equal(new[2], X[0]) and new[1, 0] == np.float32((2.0 + 3e19 + 1.0) / 3.0)
    # a row whose every distance is +inf keeps the lowest candidate, as cilrs_knn returns it
    big = np.full((1, 4), 3e19, dtype=np.float32)
    with np.errstate(over="ignore"):
        d32 = ((big - Cn[1:3]) ** 2).sum(axis=1, dtype=np.float32)
    assert np.isinf(d32).all() and KM.assign(big, Cn)[0].tolist() == [1]
    # rows labelled -1 (or outside 0..K-1) take no part in an update
    lab = np.array([0, 0, -1, 7, 1], dtype=np.int32)
    got = KM.update(X, lab, Cn[:2])
    assert np.array_equal(got[0], [1, 0, 0, 0]) and np.array_equal(got[1], [1, 0, 0, 0])


def test_planted_blobs_are_recovered_by_the_definition():
    for K, per, D, seed in ((9, 30, 260, 5), (4, 10, F0, 6)):
        X, truth = KM.blobs(K, per, D, seed)
        diam, sep = KM.blob_geometry(X, truth)
        assert sep > 2.0 * diam, (diam, sep)
        sel, radius, _m = KC.greedy(X, np.full(len(X), np.inf), K)
        assert sorted(truth[sel].tolist()) == list(range(K))                 # one row per blob
        C, label, _d, cnt, inertia, changed = KM.lloyd(X, X[sel], 3)
        assert KM.same_partition(label, truth) and (cnt == per).all()
        assert changed.tolist() == [len(X), 0, 0, 0] and inertia[1] == inertia[3] < inertia[0]
        assert not KM.same_partition(np.zeros(len(X), dtype=np.int32), truth)


# ---- FramePool.cluster with the launches replaced by the definition -----------------------------------
class _HostPool(TKH._HostPool):
    calls = 0

    def _lloyd_op(self, rows, centres, iters, labels, dist, counts, inertia, changed):
        assert rows.stride(1) == 1 and centres.is_contiguous() and labels.dtype == torch.int32
        assert inertia.numel() == changed.numel() == iters + 1
        self.calls += 1
        C, l, d, n, ine, chg = KM.lloyd(rows.numpy(), centres.numpy(), iters, labels.numpy())
        centres.copy_(torch.from_numpy(C))
        labels.copy_(torch.from_numpy(l))
        dist.copy_(torch.from_numpy(d.astype(np.float32)))
        counts.copy_(torch.from_numpy(n))
        inertia.copy_(torch.from_numpy(ine))
        changed.copy_(torch.from_numpy(chg))

    def _assign_op(self, rows, centres, labels, dist, counts, inertia, changed):
        self._lloyd_op(rows, centres, 0, labels, dist, counts, inertia, changed)

    def _update_op(self, rows, labels, centres, counts):
        centres.copy_(torch.from_numpy(KM.update(rows.numpy(), labels.numpy(), centres.numpy())))
        counts.copy_(torch.from_numpy(KM.counts(labels.numpy(), centres.size(0))))


def _blob_pool(K=4, per=10, seed=6):
    X, truth = KM.blobs(K, per, F0, seed)
    pool = _HostPool(TH._Stub(), capacity=len(X))
    pool.add_features(torch.from_numpy(X))
    return pool, X, truth


def test_cluster_three_init_forms_and_stopping():
    pool, X, truth = _blob_pool()
    c = pool.cluster(4, iters=50, check_every=5)
    assert isinstance(c, Clustering) and c.metric == "euclidean" and len(c) == 4 and c.F == F0
    assert KM.same_partition(c.labels.numpy(), truth) and c.sizes.tolist() == [10] * 4
    # stops in the first block: its second assignment found no change
    assert pool.calls == 1 and c.converged and c.iterations == 1
    assert c.changed.tolist() == [40, 0, 0, 0, 0, 0] and len(c.inertia) == 6
    assert c.labels.dtype == torch.int32 and c.dist.dtype == torch.float32 and c.sizes.dtype == np.int64
    sel = pool.select(4).indices
    want = KM.lloyd(X, X[sel], 5)
    assert np.array_equal(c.centres.numpy(), want[0]) and np.array_equal(c.labels.numpy(), want[1])
    # rows by index and centres by value: the same run
    rows = pool.cluster(4, init=torch.from_numpy(sel), iters=50, check_every=5)
    vals = pool.cluster(4, init=torch.from_numpy(X[sel]), iters=50, check_every=5)
    for o in (rows, vals):
        assert torch.equal(o.centres, c.centres) and torch.equal(o.labels, c.labels)
        assert np.array_equal(o.inertia, c.inertia)
    # blocks of one: a block's first assignment is the closing one of the block before, kept once
    pool.calls = 0
    one = pool.cluster(4, iters=50, check_every=1)
    assert pool.calls == 1 and one.changed.tolist() == [40, 0] and one.iterations == 1 and one.converged
    # seeds inside one blob need more than one block of one
    pool.calls = 0
    same = np.flatnonzero(truth == 0)[:4]
    slow = pool.cluster(4, init=torch.from_numpy(same), iters=50, check_every=1)
    ref = KM.lloyd(X, X[same], len(slow.changed) - 1)
    assert pool.calls == len(slow.changed) - 1 >= 2 and slow.converged
    assert np.array_equal(slow.changed, ref[5]) and np.array_equal(slow.inertia, ref[4])
    assert np.array_equal(slow.centres.numpy(), ref[0]) and slow.changed[-1] == 0 and (slow.changed[:-1] > 0).all()
    # iters = 0 is the closing assignment alone; iters smaller than the need: not converged
    zero = pool.cluster(4, init=torch.from_numpy(same), iters=0)
    assert zero.iterations == 0 and not zero.converged and len(zero.changed) == 1
    assert torch.equal(zero.centres, torch.from_numpy(X[same]))
    short = pool.cluster(4, init=torch.from_numpy(same), iters=1, check_every=5)
    assert short.iterations == 1 and not short.converged and len(short.changed) == 2


def test_cluster_radius_zero_cut_raises_and_an_empty_cluster_keeps_its_centre():
    X = TKH.TK._int_rows(12, F0, 4, 3)                       # four distinct rows, three times each
    pool = _HostPool(TH._Stub(), capacity=12)
    pool.add_features(torch.from_numpy(X))
    assert len(pool.cluster(4).sizes) == 4
    with pytest.raises(RuntimeError, match="distinct rows"):
        pool.cluster(5)
    far = np.concatenate([X[:3], np.full((1, F0), 1000.0, dtype=np.float32)])
    c = pool.cluster(4, init=torch.from_numpy(far), iters=3)
    assert c.sizes[3] == 0 and torch.equal(c.centres[3], torch.from_numpy(far[3]))
    w = c.balanced_weights()
    assert w.dtype == np.float64 and w.shape == (12,)
    labels = c.labels.numpy()
    live = np.flatnonzero(c.sizes > 0)
    for k in live:
        assert abs(w[labels == k].sum() - 12 / len(live)) < 1e-12
    idx = DATA.weighted_indices(w, 8, generator=torch.Generator().manual_seed(0))
    assert idx.shape == (8,) and int(idx.max()) < 12


def test_cluster_with_a_density_assign_medoids_histogram_and_round_trip(tmp_path):
    pool, fd, vt, rows = TKH._pools()
    pool = _HostPool(TH._Stub(), capacity=rows).add_features(vt[:rows])
    c = pool.cluster(6, density=fd, iters=30)
    assert c.metric == "mahalanobis" and c.commands == TH.NC0 and tuple(c.centres.shape) == (6, F0)
    index = pool.index(density=fd)
    assert torch.equal(c.rows, index.rows) and torch.equal(c.W, fd.W)       # whitened as every query is
    ref = KM.lloyd(c.rows.numpy(), c.rows.numpy()[pool.select(6, density=fd).indices], len(c.changed) - 1)
    assert np.array_equal(c.centres.numpy(), ref[0]) and np.array_equal(c.labels.numpy(), ref[1])
    assert np.array_equal(c.sizes, ref[3]) and c.sizes.sum() == rows
    labels, dist = c.assign(vt[:rows])                       # raw rows with their pad columns
    assert labels.dtype == torch.int32 and torch.equal(labels, c.labels) and torch.equal(dist, c.dist)
    assert np.array_equal(c.histogram(vt[:rows]), c.sizes)
    assert c.histogram(vt[rows:rows + 50]).sum() == 50
    med = c.medoids()
    d = KM.dist_matrix(c.rows.numpy(), c.centres.numpy())
    assert med.dtype == np.int64 and np.array_equal(med, d.argmin(axis=0))
    c.save(tmp_path / "c.pt")
    back = Clustering.load(tmp_path / "c.pt")
    back.index_class = TKH._HostIndex
    for name in ("centres", "labels", "dist", "origin", "W"):
        assert torch.equal(getattr(back, name), getattr(c, name)), name
    for name in ("sizes", "inertia", "changed"):
        assert np.array_equal(getattr(back, name), getattr(c, name)), name
    assert (back.metric, back.iterations, back.converged, back.K) == (c.metric, c.iterations, c.converged, 6)
    assert torch.equal(back.assign(vt[:rows])[0], c.labels)
    assert np.array_equal(back.medoids(c.rows), med)
    with pytest.raises(RuntimeError, match="rows"):
        back.medoids()
    with pytest.raises(RuntimeError, match="features"):
        Clustering(torch.zeros(2, F0 * 2), None, None, [0, 0], [], [], 0, False).load_state_dict(c.state_dict())
    # float32 centres are whitened first
    raw = vt[:6, :F0].clone()
    v = pool.cluster(6, density=fd, init=raw, iters=0)
    assert torch.equal(v.centres, index.whiten(raw))


def test_cluster_refusals():
    stub = TH._Stub()
    pool = _HostPool(stub, capacity=8)
    with pytest.raises(RuntimeError, match="empty"):
        pool.cluster(1)
    X = torch.from_numpy(KC.relu_rows(6, F0, 1))
    pool.add_features(X)
    for k in (0, 7, -2):
        with pytest.raises(ValueError, match="k must be"):
            pool.cluster(k)
    big = _HostPool(stub, capacity=1100).add_features(torch.zeros(1100, F0))
    with pytest.raises(ValueError, match="k must be"):
        big.cluster(1025)
    for bad in (-1, 10001):
        with pytest.raises(ValueError, match="iters"):
            pool.cluster(2, iters=bad)
    with pytest.raises(ValueError, match="check_every"):
        pool.cluster(2, check_every=0)
    for bad in ("random", torch.zeros(3, dtype=torch.int64), torch.tensor([0, 6]), torch.zeros(2, F0 - 4),
                torch.zeros(3, F0), torch.zeros(2, F0, dtype=torch.float64)):
        with pytest.raises(ValueError, match="init"):
            pool.cluster(2, init=bad)
    with pytest.raises(RuntimeError, match="finalize"):
        pool.cluster(2, density=TH._HostDensity(stub))
    fd, _vt, _ct, _rows = TH._fitted(rows=100)
    fd.finalize()
    with pytest.raises(RuntimeError, match="features"):
        _HostPool(TH._Stub(F=2 * F0), capacity=4).add_features(torch.zeros(2, 2 * F0)).cluster(1, density=fd)
    assert pool.calls == 0                                   # nothing was launched
    # without a device there is no fallback
    plain = FramePool(stub, capacity=8).add_features(X)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.cluster(2, init=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="metric"):
        Clustering(torch.zeros(2, F0), None, None, [0, 0], [], [], 0, False, metric="cosine")
