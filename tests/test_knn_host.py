"""K nearest neighbours on the host: the float64 definition (tests/_knn.py) against a brute-force
sort, the whitened coordinates, statistical sanity of the k-th neighbour score, and
cilrs_mi355.neighbours.NeighbourIndex with its launches replaced by the definition.

Bounds.  Whitening: |W (a - b)|^2 = (a - b)^T Sigma_l^-1 (a - b) holds exactly for W = L^-1,
Sigma_l = L L^T; gated at 1e-10 relative as test_kcenter_host.py gates it (its docstring).  The
percentile of a log's own median: searchsorted(side="right") of the element of rank r (from 0) in a
sorted log of n scores is 100 (r + 1) / n, 50 exactly at r = n / 2 - 1, plus one rank where the next
score equals it -- two rows that are each other's k-th neighbour log the same distance, so scores tie
in pairs -- hence 50 +- 100 / n.
Sanity: N = 2,000 unit Gaussian rows at F = 16, k = 8, 200 fresh rows against 200 shifted along one
axis, all 40,000 pairs.  Measured with the float64 definition before this test was written: a shift
of 3 sigma gives 0.79 .. 0.81 of all pairs (0.89 .. 0.91 of the 200 same-noise pairs) over four seeds
-- in 16 dimensions the k-th neighbour distance of an in-distribution row already spreads that widely
-- 4 sigma 0.92, 5 sigma 0.976 .. 0.980.  The test uses 5 sigma, seed 0 (0.976), gate 0.95.
"""
import numpy as np
import pytest
import torch

import _kcenter as KC
import _knn as KN
import _novelty as N
import test_kcenter_host as TK
import test_novelty_host as TH
from cilrs_mi355 import FramePool, NeighbourIndex

F0 = TH.F0


# ---- the definition -----------------------------------------------------------------------------------
def _int_rows(n, d, seed, top=3):
    return np.random.default_rng(seed).integers(0, top, size=(n, d)).astype(np.float32)


@pytest.mark.parametrize("n,d,K", [(1, 4, 3), (3, 4, 5), (40, 4, 1), (40, 4, 7), (40, 8, 40), (40, 8, 64)])
def test_definition_against_a_brute_force_sort(n, d, K):
    X = _int_rows(n, d, 5 * n + d)
    if n >= 40:
        X[20:30] = X[0:10]                                   # duplicates: ties in d
        X[7] = np.nan                                        # a NaN row is never a candidate
        X[11, 1] = np.nan
    Y = np.concatenate([_int_rows(5, d, 99), X[:2]])
    assert np.isfinite(Y).all()
    for skip in (None, np.array([-1, 0, n - 1, n, 1 << 40, 0, 1])):
        idx, dist = KN.knn(X, Y, K, skip)
        bi, bd = KN.brute(X, Y, K, skip)
        assert np.array_equal(idx, bi) and np.array_equal(dist, bd)
        cand = n - (2 if n >= 40 else 0)
        for q in range(len(Y)):
            here = cand - (1 if skip is not None and 0 <= skip[q] < n and
                           np.isfinite(X[skip[q]]).all() else 0)
            assert (idx[q, here:] == -1).all() and np.isinf(dist[q, here:]).all()
            assert (idx[q, :min(here, K)] >= 0).all()
            if skip is not None and 0 <= skip[q] < n:
                assert int(skip[q]) not in idx[q].tolist()
            assert 7 not in idx[q].tolist() and 11 not in idx[q].tolist()
    if n >= 40 and K >= 2:
        # the (d, i) tie rule: query 5 is row 0, which row 20 repeats
        idx, dist = KN.knn(X, Y, K)
        assert idx[5, :2].tolist() == [0, 20] and not dist[5, :2].any()
        assert KN.knn(X, Y, K, np.full(7, 0))[0][5, 0] == 20


def test_order_keeps_infinities_and_the_dtype():
    d = np.array([np.inf, 2.0, np.nan, np.inf, 2.0], dtype=np.float32)
    idx, dist = KN.order(d, 6)
    assert idx.tolist() == [1, 4, 0, 3, -1, -1] and dist.dtype == np.float32
    assert dist.tolist() == [2.0, 2.0, np.inf, np.inf, np.inf, np.inf]
    assert KN.order(d, 2, skip=1)[0].tolist() == [4, 0]
    assert KN.order(np.full(3, np.nan), 2)[0].tolist() == [-1, -1]
    # K = 8 is the prefix of K = 64
    X, Y = KC.relu_rows(100, 12, 1), KC.relu_rows(3, 12, 2)
    a, b = KN.knn(X, Y, 8), KN.knn(X, Y, 64)
    assert np.array_equal(a[0], b[0][:, :8]) and np.array_equal(a[1], b[1][:, :8])


def test_whitened_distance_is_the_quadratic_form():
    fd, vt, _ct, rows = TH._fitted()
    fd.finalize()
    v = vt[:rows, :F0].numpy()
    fin = N.finalize(fd.table.numpy(), fd.pivot.numpy(), F0, TH.NC0, TH.LAM)
    k0 = int(np.flatnonzero(fin["present"])[0])
    white = lambda x: (x.astype(np.float64) - fin["mean"][k0]) @ np.tril(fin["W"]).T
    a, b = v[:80], v[80:160]
    got = ((white(a) - white(b)) ** 2).sum(axis=1)
    u = a.astype(np.float64) - b.astype(np.float64)
    want = np.einsum("bi,bi->b", u, np.linalg.solve(fin["sigma_l"], u.T).T)
    rel = np.abs(got - want).max() / want.max()
    print(f"|whiten(a) - whiten(b)|^2 against the quadratic form: {rel:.3g}")
    assert rel <= 1e-10


def test_kth_neighbour_score_separates_shifted_gaussian_rows():
    rng = np.random.default_rng(0)
    F, n, M, k, shift = 16, 2000, 200, 8, 5.0
    X = rng.standard_normal((n, F)).astype(np.float32)
    fresh = rng.standard_normal((M, F)).astype(np.float32)
    shifted = fresh.copy()
    shifted[:, 0] += shift
    index = _HostIndex(torch.from_numpy(X))
    a, b = index.score(torch.from_numpy(fresh), k).numpy(), index.score(torch.from_numpy(shifted), k).numpy()
    share = float((a[:, None] < b[None, :]).mean())
    print(f"k = {k} score: in-distribution mean {a.mean():.3f}, shifted by {shift} sigma {b.mean():.3f}; "
          f"{share:.4f} of the {M * M} pairs in order")
    assert share >= 0.95


# ---- NeighbourIndex with the launches replaced by the definition -----------------------------------
class _HostIndex(NeighbourIndex):
    def _whiten_op(self, features, y):
        z, _ = KN.whiten64(features[:, :self.F].numpy(), self.origin.numpy(), self.W.numpy())
        y.copy_(torch.from_numpy(z.astype(np.float32)))

    def _knn_op(self, queries, k, skip, idx, dist):
        assert queries.stride(1) == 1 and idx.is_contiguous() and dist.is_contiguous()
        i, d = KN.knn(self.rows.numpy(), queries[:, :self.F].numpy(), k,
                      None if skip is None else skip.numpy())
        idx.copy_(torch.from_numpy(i))
        dist.copy_(torch.from_numpy(d.astype(np.float32)))


class _HostPool(TK._HostPool):
    index_class = _HostIndex


def _pools():
    fd, vt, _ct, rows = TH._fitted()
    fd.finalize()
    pool = _HostPool(TH._Stub(), capacity=rows)
    pool.add_features(vt[:rows])                             # ld = F + 8, the pad columns NaN
    return pool, fd, vt, rows


def test_index_returns_a_pool_row_first_at_distance_zero():
    pool, fd, vt, rows = _pools()
    for index in (pool.index(), pool.index(density=fd)):
        assert isinstance(index, _HostIndex) and len(index) == rows and index.F == F0
        assert index.metric == ("euclidean" if index.W is None else "mahalanobis")
        pick = torch.tensor([0, 17, rows - 1])
        idx, dist = index.query(vt[pick], 5)                 # raw rows with their pad columns
        assert idx.dtype == torch.int64 and dist.dtype == torch.float32
        assert tuple(idx.shape) == tuple(dist.shape) == (3, 5)
        assert torch.equal(idx[:, 0], pick) and not dist[:, 0].any()
        assert bool((dist[:, 1:] > 0).all()) and bool((dist[:, 1:] >= dist[:, :-1]).all())
        i2, d2 = index.query(vt[pick], 5, skip=pick)         # leave-one-out
        assert not (i2 == pick[:, None]).any()
        assert torch.equal(i2[:, :4], idx[:, 1:]) and torch.equal(d2[:, :4], dist[:, 1:])
        one = index.query(vt[17, :F0], 3)                    # a single vector
        assert one[0].tolist() == [idx[1, :3].tolist()]
        assert torch.equal(index.score(vt[pick], 5), dist[:, 4])
        assert tuple(index.query(vt[:0], 4)[0].shape) == (0, 4)
    # the whitened rows are the definition's, and the pool is copied, not viewed
    mah = pool.index(density=fd)
    k0 = int(np.flatnonzero(fd.present)[0])
    z, _ = KN.whiten64(vt[:rows, :F0].numpy(), fd.mean.numpy()[k0], fd.W.numpy())
    assert np.array_equal(mah.rows.numpy(), z.astype(np.float32))
    assert torch.equal(mah.origin, fd.mean[k0]) and torch.equal(mah.W, fd.W) and mah.commands == TH.NC0
    euc = pool.index()
    pool.pool.zero_()
    assert torch.equal(euc.rows, vt[:rows, :F0])


def test_calibrate_percentile_and_round_trip(tmp_path):
    pool, fd, vt, rows = _pools()
    index = pool.index(density=fd)
    with pytest.raises(RuntimeError, match="no calibration"):
        index.quantile(0.5)
    assert index.calibrate(4) is index and index.log_count == rows and index.log_k == 4
    s = index.calibration_scores()
    assert s.shape == (rows,) and (np.diff(s) >= 0).all() and (s > 0).all()
    loo = index._query_rows(index.rows, 4, torch.arange(rows))[1][:, 3].numpy()
    assert np.array_equal(np.sort(loo), s)
    med = s[rows // 2 - 1]
    assert (s == med).sum() <= 2, "the bound of the docstring: scores tie in pairs at the most"
    assert abs(index.percentile(float(med)) - 50.0) <= 100.0 / rows
    assert index.quantile(0.0) == s[0] and index.quantile(1.0) == s[-1]
    pc = index.percentile(np.linspace(0.0, 2.0 * float(s[-1]), 40, dtype=np.float32))
    assert (np.diff(pc) >= 0).all() and pc[0] == 0.0 and pc[-1] == 100.0
    index.calibrate(4, rows=[3, 5])                          # the same k: the log goes on
    assert index.log_count == rows + 2
    index.calibrate(2, rows=torch.tensor([3, 5, 9]))         # another k starts it again
    assert index.log_count == 3 and index.log_k == 2
    with pytest.raises(ValueError, match="rows"):
        index.calibrate(2, rows=[rows])
    # save / load reproduces query exactly
    want = index.query(vt[rows:rows + 9], 6)
    for idx_, name in ((index, "mah.pth"), (pool.index(), "euc.pth")):
        path = tmp_path / name
        idx_.save(path)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert set(sd) == {"F", "N", "metric", "weights_key", "commands", "rows", "origin", "W",
                           "calibration", "calibration_k"}
        back = _HostIndex.load(path)
        assert back.metric == idx_.metric and len(back) == rows and back.log_k == idx_.log_k
        a, b = idx_.query(vt[rows:rows + 9], 6), back.query(vt[rows:rows + 9], 6)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if idx_.log_count:
            assert np.array_equal(back.calibration_scores(), idx_.calibration_scores())
    assert torch.equal(want[0], index.query(vt[rows:rows + 9], 6)[0])


def test_index_refusals():
    pool, fd, vt, rows = _pools()
    index = pool.index()
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be"):
            index.query(vt[:2], k)
    for bad in (vt[:2].double(), vt[:2, :F0 - 4], vt[:2, None]):
        with pytest.raises(RuntimeError, match="float32"):
            index.query(bad, 2)
    with pytest.raises(RuntimeError, match="skip"):
        index.query(vt[:3], 2, skip=[0, 1])
    with pytest.raises(RuntimeError, match="features"):
        index.check_model(TH._Stub(F=2 * F0))
    index.check_model(TH._Stub())
    with pytest.raises(RuntimeError, match="commands"):
        pool.index(density=fd).check_model(TH._Stub(NC=TH.NC0 + 1))
    with pytest.raises(RuntimeError, match="empty"):
        _HostPool(TH._Stub(), capacity=4).index()
    with pytest.raises(RuntimeError, match="finalize"):
        pool.index(density=TH._HostDensity(TH._Stub()))
    with pytest.raises(ValueError, match="metric"):
        NeighbourIndex(vt[:4, :F0], "cosine")
    with pytest.raises(ValueError, match="origin and W"):
        NeighbourIndex(vt[:4, :F0], "mahalanobis")
    # without a device there is no fallback
    plain = FramePool(TH._Stub(), capacity=8).add_features(vt[:6])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.index().query(vt[:2], 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.index(density=fd)
