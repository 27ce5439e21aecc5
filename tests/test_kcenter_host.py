"""Greedy k-center on the host: properties of the float64 definition (tests/_kcenter.py), the
whitened coordinates of FeatureDensity, and cilrs_mi355.select.FramePool with its launches replaced
by the definition.

Bounds.  The 2-approximation is the textbook guarantee of farthest-point selection (Gonzalez, 1985)
on true distances, so 4 on the squared ones; both sides are float64 sums of two squares, compared
with a 1e-12 relative margin.  Whitening: the identity |W (a - b)|^2 = (a - b)^T Sigma_l^-1 (a - b)
holds exactly for W = L^-1, Sigma_l = L L^T; numpy's float64 leaves cond(Sigma_l) 2^-53 <= 6.4e3 *
1.1e-16 < 1e-12 of it (test_novelty_host.py, docstring), gated at 1e-10 relative as there.
FeatureDensity.whiten is an fp32 product of F terms: (F + 2) 2^-24 sum_j |W_ij||u_j| per entry.
"""
import itertools

import numpy as np
import pytest
import torch

import _kcenter as K
import _novelty as N
import test_novelty_host as TH
from cilrs_mi355 import FramePool, Selection
from cilrs_mi355.novelty import FeatureDensity

F0 = TH.F0


def test_radius_is_non_increasing_and_mind_of_a_pick_is_zero():
    for seed, (n, d) in enumerate([(40, 8), (7, 4), (300, 12)]):
        X = K.relu_rows(n, d, seed)
        sel, radius, m = K.greedy(X, np.full(n, np.inf), min(n, 25))
        assert sel[0] == 0 and radius[0] == np.inf
        assert (np.diff(radius) <= 0).all()
        assert (m[sel] == 0).all() and len(set(sel.tolist())) == len(sel)
        assert radius[-1] >= m.max()
        # K1 picks then K2 more on the same mind are K1 + K2 picks
        s1, r1, m1 = K.greedy(X, np.full(n, np.inf), 3)
        s2, r2, m2 = K.greedy(X, m1, min(n, 25) - 3)
        assert np.array_equal(np.concatenate([s1, s2]), sel) and np.array_equal(m2, m)
        assert np.array_equal(np.concatenate([r1, r2]), radius)


def test_nan_entries_never_win_and_a_nan_in_front_is_never_beaten():
    m = np.array([1.0, np.nan, 3.0, 3.0, np.nan])
    assert K.argmax_low(m) == 2
    assert K.argmax_low(np.array([np.nan, 5.0])) == 0
    assert K.argmax_low(np.array([np.inf, np.inf])) == 0
    assert np.array_equal(K.lower(np.array([1.0, 2.0]), np.array([np.nan, 1.5])), [1.0, 1.5])


@pytest.mark.parametrize("seed", range(6))
def test_greedy_radius_is_within_twice_the_optimum(seed):
    n, k, d = 9, 3, 2
    X = K.relu_rows(n, d, 100 + seed) + np.random.default_rng(seed).standard_normal((n, d)).astype(
        np.float32)
    _sel, _radius, m = K.greedy(X, np.full(n, np.inf), k)
    greedy = m.max()
    sets = list(itertools.combinations(range(n), k))
    assert len(sets) == 84
    best = min(K.cover(X, X[list(s)], np.full(n, np.inf)).max() for s in sets)
    print(f"seed {seed}: greedy radius^2 {greedy:.6g}, optimum {best:.6g}, ratio of radii "
          f"{np.sqrt(greedy / best):.3f}")
    assert best <= greedy * (1 + 1e-12) and greedy <= 4.0 * best * (1 + 1e-12)


def test_whitened_distance_is_the_mahalanobis_distance():
    fd, vt, _ct, rows = TH._fitted()
    fd.finalize()
    v = vt[:rows, :F0].numpy()
    fin = N.finalize(fd.table.numpy(), fd.pivot.numpy(), F0, TH.NC0, TH.LAM)
    k0 = int(np.flatnonzero(fin["present"])[0])
    white = lambda x: (x.astype(np.float64) - fin["mean"][k0]) @ np.tril(fin["W"]).T
    a, b = v[:60], v[60:120]
    got = ((white(a) - white(b)) ** 2).sum(axis=1)
    u = a.astype(np.float64) - b.astype(np.float64)
    want = np.einsum("bi,bi->b", u, np.linalg.solve(fin["sigma_l"], u.T).T)
    rel = np.abs(got - want).max() / want.max()
    print(f"|whiten(a) - whiten(b)|^2 against the quadratic form: {rel:.3g}")
    assert rel <= 1e-10
    # the fp32 product of FeatureDensity.whiten against float64 of the same rounded tables
    W32, m32 = fd.W.numpy().astype(np.float64), fd.mean.numpy()
    u32 = (v - m32[k0]).astype(np.float64)                   # the fp32 difference, as whiten takes it
    ref = u32 @ np.tril(W32).T
    bound = (F0 + 2) * 2.0 ** -24 * (np.abs(u32) @ np.abs(np.tril(W32)).T)
    z = fd.whiten(vt[:rows])                                 # ld = F + 8, the pad columns NaN
    assert z.dtype == torch.float32 and tuple(z.shape) == (rows, F0)
    err = np.abs(z.numpy() - ref)
    print(f"whiten fp32: largest share of the bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all()
    zm = fd.whitened_means()
    assert tuple(zm.shape) == (int(fd.present.sum()), F0) and not zm[0].any()
    with pytest.raises(RuntimeError, match="finalize"):
        TH._HostDensity(TH._Stub()).whiten(vt[:2])
    with pytest.raises(RuntimeError, match="float32"):
        fd.whiten(vt[:2, :F0 - 1])


# ---- FramePool with the launches replaced by the definition ----------------------------------------
class _HostPool(FramePool):
    def _cover_op(self, rows, centres, mind):
        assert rows.stride(1) == 1 and centres.stride(1) == 1
        m = K.cover(rows.numpy(), centres.numpy(), mind.numpy())
        mind.copy_(torch.from_numpy(m.astype(np.float32)))

    def _greedy_op(self, rows, mind, k):
        sel, radius, m = K.greedy(rows.numpy(), mind.numpy(), k)
        mind.copy_(torch.from_numpy(m.astype(np.float32)))
        return torch.from_numpy(sel), torch.from_numpy(radius.astype(np.float32))


def _int_rows(n, d, distinct, seed):
    """rows with integer entries 0..7, `distinct` different ones repeated in turn"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 8, size=(distinct, d)).astype(np.float32)
    assert len({r.tobytes() for r in base}) == distinct
    return base[np.arange(n) % distinct]


def test_selection_is_cut_at_the_first_zero_radius():
    X = _int_rows(12, F0, 4, 3)
    pool = _HostPool(TH._Stub(), capacity=12)
    pool.add_features(torch.from_numpy(X[:5])).add_features(torch.from_numpy(X[5:]))
    assert len(pool) == 12 and torch.equal(pool.features(), torch.from_numpy(X))
    s = pool.select(6)
    assert isinstance(s, Selection) and s.metric == "euclidean"
    assert s.indices.dtype == np.int64 and s.radius.dtype == np.float32
    assert len(s.indices) == len(s.radius) == 4 and s.indices[0] == 0 and s.radius[0] == np.inf
    assert sorted((s.indices % 4).tolist()) == [0, 1, 2, 3] and (s.indices < 4).all()
    assert not s.min_dist.any() and s.min_dist.shape == (12,)
    assert np.array_equal(s.coverage(), np.sqrt(s.radius)) and (np.diff(s.radius) <= 0).all()
    # another first centre; the same rows covered beforehand leave nothing to pick
    s5 = pool.select(3, first=5)
    assert s5.indices[0] == 5 and s5.radius[0] == np.inf and len(s5.indices) == 3
    assert 1 not in (s5.indices[1:] % 4)
    assert len(pool.select(1, first=7).indices) == 1
    none = pool.select(3, covered=torch.from_numpy(X[:4]))
    assert len(none.indices) == 0 and not none.min_dist.any()
    part = pool.select(5, covered=torch.from_numpy(X[1:3]))
    assert sorted((part.indices % 4).tolist()) == [0, 3]


def test_selection_with_a_density_covers_the_command_means():
    fd, vt, _ct, rows = TH._fitted()
    fd.finalize()
    pool = _HostPool(TH._Stub(), capacity=rows)
    pool.add_features(vt[:rows])                             # ld = F + 8: only the features are kept
    s = pool.select(10, density=fd)
    assert s.metric == "mahalanobis" and len(s.indices) == 10 and np.isfinite(s.radius).all()
    Z = fd.whiten(pool.features()).numpy()
    m0 = K.cover(Z, fd.whitened_means().numpy(), np.full(rows, np.inf))
    sel, radius, m = K.greedy(Z, m0.astype(np.float32), 10)
    assert np.array_equal(s.indices, sel) and np.array_equal(s.radius, radius.astype(np.float32))
    assert torch.equal(s.rows, fd.whiten(pool.features()))
    again = pool.select(5, density=fd, covered=vt[torch.from_numpy(s.indices)])
    assert not set(again.indices.tolist()) & set(s.indices.tolist())
    assert again.radius[0] <= s.radius[-1]


def test_frame_pool_refusals():
    stub = TH._Stub()
    with pytest.raises(RuntimeError, match="fp32 only"):
        FramePool(stub, 8, half=True)
    for cap in (0, -1, (1 << 24) + 1):
        with pytest.raises(ValueError, match="capacity"):
            FramePool(stub, cap)
    pool = _HostPool(stub, capacity=8)
    with pytest.raises(RuntimeError, match="empty"):
        pool.select(1)
    X = torch.from_numpy(K.relu_rows(6, F0, 1))
    for bad in (X.double(), X[:, :F0 - 4], X[0]):
        with pytest.raises(RuntimeError, match="float32"):
            pool.add_features(bad)
    pool.add_features(X)
    with pytest.raises(RuntimeError, match="full"):
        pool.add_features(X[:3])
    assert len(pool) == 6
    for k in (0, 7, -2):
        with pytest.raises(ValueError, match="k must be"):
            pool.select(k)
    with pytest.raises(RuntimeError, match="finalize"):
        pool.select(2, density=TH._HostDensity(stub))
    fd, _vt, _ct, _rows = TH._fitted(rows=100)
    fd.finalize()
    with pytest.raises(RuntimeError, match="features"):
        _HostPool(TH._Stub(F=2 * F0), capacity=4).add_features(torch.zeros(2, 2 * F0)).select(
            1, density=fd)
    for bad in (X.double(), X[:, :F0 - 4], X[0]):
        with pytest.raises(RuntimeError, match="covered"):
            pool.select(2, covered=bad)
    with pytest.raises(ValueError, match="first"):
        pool.select(2, covered=X[:1], first=1)
    with pytest.raises(ValueError, match="first"):
        pool.select(2, density=fd, first=1)
    for first in (-1, 6):
        with pytest.raises(ValueError, match="first"):
            pool.select(2, first=first)
    pool.clear()
    assert len(pool) == 0
    # without a device there is no fallback
    plain = FramePool(stub, capacity=8).add_features(X)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.select(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.select(2, covered=X[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.add(torch.zeros(1, 3, 40, 120), torch.zeros(1), torch.zeros(1, dtype=torch.int64))
