"""Bulk k-NN on the matrix cores (csrc/knn_join.hip: cilrs_knn_join; NeighbourIndex.join / graph /
calibrate(bulk=True); FramePool.nearest / novel_rows / select(covered_index=)) against the definition
of include/cilrs_hip.h ("Bulk nearest neighbours").

Gates.  Op level, bit-exact: every query the entry certifies carries the (idx, dist) the device's own
cilrs_knn gives for it (np.array_equal on the integers and on the distances' bits); every other query
holds -2 / NaN in all K slots; n_uncertified is the sum of the flags; a second call repeats outputs
and flags bit for bit; a query's row does not depend on its place in the call or on the call it is
in.  The fast path is really taken: every query for which tests/_knn_join.py must_certify holds (a
float64 predicate with the header's b, E_q and K_s = K + 8) has to come back certified.  Python level:
join / graph / calibrate(bulk=True) equal query / calibrate with torch.equal, also where everything
falls back.

What the cases cross.  The screen's workgroup owns TQ = 128 queries and walks the pool in tiles of
TN = 128 rows, staged in D-chunks of 16 columns (D = 4, 12, 36, 260, 516 end in a partial chunk; the
pad columns of X and Y hold NaN).  With few query tiles the pool's tiles are cut into slices, one
workgroup each: N = 2 TN + 5 and 1,030 with Q <= 2 TQ + 3 are three and nine slices of one tile.
Outputs are pre-filled (idx -7, dist NaN, flags -7) inside guard bands (tests/_guards.py) and the
scratch is exactly cilrs_knn_join_scratch_bytes.
"""
import numpy as np
import pytest
import torch

import _guards as G
import _kcenter as KC
import _knn_join as KJ
import test_kcenter_gpu as TK
import test_knn_gpu as TKN
import test_mc_dropout_gpu as TM
import test_novelty_gpu as TN

pytestmark = pytest.mark.gpu

TQ, TN_ROWS, CHUNK = 128, 128, 16         # csrc/knn_join.hip: kJoinTQ, kJoinTN, kJoinKC
GROUPS = 512                              # kJoinGroups: workgroups the slices aim at
_CACHE = {}

_lib, _st, _err, _dev_rows = TKN._lib, TK._st, TK._err, TK._dev_rows
_same_bits = TKN._same_bits


def slices(N, Q):
    """join_split of csrc/knn_join.hip"""
    nt, qt = -(-N // TN_ROWS), -(-Q // TQ)
    want = min(nt, max(1, -(-GROUPS // qt)))
    tps = -(-nt // want)
    return -(-nt // tps)


class _Out:
    """guarded idx (-7) / dist (NaN) / flags (-7) / count (-7) and an exactly sized scratch"""

    def __init__(self, N, Q, D, K, short=0):
        self.nbytes = _lib().lib().cilrs_knn_join_scratch_bytes(N, Q, D, K)
        self.idx, c1 = G.guarded(Q * K, dtype=torch.int64, fill=-7, name="idx")
        self.dist, c2 = G.guarded(Q * K, name="dist")
        self.unc, c3 = G.guarded(Q, dtype=torch.int32, fill=-7, name="uncertified")
        self.cnt, c4 = G.guarded(1, dtype=torch.int32, fill=-7, name="n_uncertified")
        self.scratch, c5 = G.guarded(max(self.nbytes - short, 1), dtype=torch.uint8, fill=0xA5, name="scratch")
        self.checks = (c1, c2, c3, c4, c5)
        self.Q, self.K = Q, K

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        assert bool((self.idx == -7).all()) and bool(torch.isnan(self.dist).all()) and \
            bool((self.unc == -7).all()) and int(self.cnt[0]) == -7 and \
            bool((self.scratch == 0xA5).all()), "a refused call wrote to its outputs"

    def host(self):
        return (self.idx.view(self.Q, self.K).cpu().numpy(), self.dist.view(self.Q, self.K).cpu().numpy(),
                self.unc.cpu().numpy(), int(self.cnt[0]))


def _join(X_d, N, D, Y_d, Q, K, skip=None):
    """one guarded call; (idx, dist, flags, count) on the host after every band was checked"""
    L = _lib()
    out = _Out(N, Q, D, K)
    skip_d = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.int64)).cuda()
    ins = G.Inputs(X=X_d, Y=Y_d, skip=skip_d)
    L.check(L.lib().cilrs_knn_join(L.ptr(X_d), X_d.stride(0), N, D, L.ptr(Y_d), Y_d.stride(0), Q,
                                   L.ptr(skip_d), K, L.ptr(out.idx), L.ptr(out.dist), L.ptr(out.unc),
                                   L.ptr(out.cnt), L.ptr(out.scratch), out.nbytes, _st()))
    out.check()
    ins.check()
    return out.host()


def _against_knn(got, want, what):
    """the gates of the docstring for one call; returns the certified mask"""
    idx, dist, unc, cnt = got
    want_i, want_d = want
    assert set(np.unique(unc)) <= {0, 1}, (what, np.unique(unc))
    assert cnt == int(unc.sum()), (what, cnt, int(unc.sum()))
    ok = unc == 0
    assert np.array_equal(idx[ok], want_i[ok]), (what, np.flatnonzero((idx != want_i).any(axis=1) & ok)[:8])
    assert _same_bits(dist[ok], want_d[ok]), what
    assert (idx[~ok] == -2).all() and np.isnan(dist[~ok]).all(), what
    return ok


def _case(N, Q, D, K, with_skip, seed):
    X = KC.relu_rows(N, D, seed)
    Y, rows = TKN._queries(X, Q, seed + 1)
    skip = None
    if with_skip:
        skip = rows.copy()                        # -1 (outside 0..N-1) for the queries that are no pool rows
        skip[-1] = N + 5                          # outside on the other side
    return X, Y, skip


# one factor at a time around (N, Q, D, K) = (2 TN + 5, TQ + 1, 36, 2)
BASE = (2 * TN_ROWS + 5, TQ + 1, 36, 2)
NS = (1, 3, TN_ROWS - 1, TN_ROWS, TN_ROWS + 1, 2 * TN_ROWS + 5, 1030)
QS = (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3)
DS = (4, 12, 36, 256, 260, 512, 516, 2048)
KS = (1, 2, 15, 16)
CASES = sorted({(n, BASE[1], BASE[2], BASE[3]) for n in NS} | {(BASE[0], q, BASE[2], BASE[3]) for q in QS} |
               {(BASE[0], BASE[1], d, BASE[3]) for d in DS} | {(BASE[0], BASE[1], BASE[2], k) for k in KS} |
               {(3, TQ, 12, 16), (1030, 2 * TQ + 3, 516, 15), (TN_ROWS + 1, 1, 2048, 1)})


@pytest.mark.parametrize("N,Q,D,K", CASES, ids=[f"n{n}_q{q}_d{d}_k{k}" for n, q, d, k in CASES])
def test_entry_against_cilrs_knn(N, Q, D, K):
    assert slices(2 * TN_ROWS + 5, TQ + 1) == 3 and slices(1030, 2 * TQ + 3) == 9
    assert _lib().lib().cilrs_knn_join_candidates(K) == KJ.candidates(K)
    for with_skip in (False, True):
        what = (N, Q, D, K, with_skip)
        X, Y, skip = _case(N, Q, D, K, with_skip, 7 * N + D + K)
        X_d, Y_d = _dev_rows(X, 4), _dev_rows(Y, 8)
        want = TKN._knn(X_d, N, D, Y_d, Q, K, skip)
        got = _join(X_d, N, D, Y_d, Q, K, skip)
        ok = _against_knn(got, want, what)
        must = KJ.must_certify(X, Y, K, skip)
        assert ok[must].all(), (what, "left to the fallback:", np.flatnonzero(must & ~ok)[:8])
        print(f"{what}: {int(ok.sum())} of {Q} certified, {int(must.sum())} had to be")
        again = _join(X_d, N, D, Y_d, Q, K, skip)
        assert np.array_equal(got[0], again[0]) and _same_bits(got[1], again[1]) and \
            np.array_equal(got[2], again[2]) and got[3] == again[3], what


def test_a_query_does_not_depend_on_its_call():
    """the same queries in another order, and split over two calls of other sizes: idx, dist and
    the flag of every query stay"""
    N, Q, D, K = 1030, 2 * TQ + 3, 260, 8
    X, Y, skip = _case(N, Q, D, K, True, 5)
    Y[1, 0] = np.nan                              # a query that is not certified
    X_d = _dev_rows(X, 4)
    idx, dist, unc, _cnt = _join(X_d, N, D, _dev_rows(Y, 4), Q, K, skip)
    assert 0 < unc.sum() < Q
    perm = np.random.default_rng(0).permutation(Q)
    pi, pd, pu, _c = _join(X_d, N, D, _dev_rows(Y[perm], 4), Q, K, skip[perm])
    assert np.array_equal(pi, idx[perm]) and _same_bits(pd, dist[perm]) and np.array_equal(pu, unc[perm])
    cut = TQ - 29                                 # every query moves to another lane, wave or workgroup
    for lo, hi in ((0, cut), (cut, Q)):
        si, sd, su, _c = _join(X_d, N, D, _dev_rows(Y[lo:hi], 4), hi - lo, K, skip[lo:hi])
        assert np.array_equal(si, idx[lo:hi]) and _same_bits(sd, dist[lo:hi]) and np.array_equal(su, unc[lo:hi])


FAST = {
    "n1030_d512_k8_seed0": (1030, 512, 8, 0, False),
    "n1030_d512_k8_seed1": (1030, 512, 8, 1, False),
    "n1030_d512_k8_seed2": (1030, 512, 8, 2, False),
    "n1030_d512_k16": (1030, 512, 16, 0, False),
    "n1030_d512_k1": (1030, 512, 1, 0, False),
    "self_join_130": (130, 512, 8, 0, True),
    "n600_d2048_k8": (600, 2048, 8, 0, False),
    "n300_d4_k8": (300, 4, 8, 0, False),
}


@pytest.mark.parametrize("name", list(FAST))
def test_the_fast_path_is_taken(name):
    """an implementation that lets everything fall back fails here: on relu-Gaussian rows the
    must-certify predicate holds for all 64 queries of every case but the last (63 there)"""
    N, D, K, seed, self_join = FAST[name]
    X = KC.relu_rows(N, D, seed)
    if self_join:
        Q, Y, skip = N, X.copy(), np.arange(N, dtype=np.int64)
    else:
        Q, Y, skip = 64, KC.relu_rows(64, D, seed + 100), None
    must = KJ.must_certify(X, Y, K, skip)
    print(f"{name}: the predicate holds for {int(must.sum())} of {Q}")
    if name != "n300_d4_k8":
        assert must.all(), np.flatnonzero(~must)
    else:
        assert must.sum() >= Q // 2
    X_d, Y_d = _dev_rows(X, 4), _dev_rows(Y, 4)
    got = _join(X_d, N, D, Y_d, Q, K, skip)
    ok = _against_knn(got, TKN._knn(X_d, N, D, Y_d, Q, K, skip), name)
    assert ok[must].all(), (name, np.flatnonzero(must & ~ok))
    if name != "n300_d4_k8":
        assert got[3] == 0


# ---- Python: join is query ---------------------------------------------------------------------------
def _index(X, metric="euclidean"):
    from cilrs_mi355 import NeighbourIndex
    rows = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    if metric == "euclidean":
        return NeighbourIndex(rows)
    _m, _W, mean_d, W_d = TN._tables(X.shape[1], 4)
    return NeighbourIndex(rows, "mahalanobis", mean_d[1].contiguous(), W_d, whitened=False)


def _join_is_query(index, Y, k, skip=None):
    """join == query with torch.equal; returns last_join"""
    Y_d = torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    ji, jd = index.join(Y_d, k, skip=skip)
    qi, qd = index.query(Y_d, k, skip=skip)
    torch.cuda.synchronize()
    assert torch.equal(ji, qi), np.flatnonzero((ji != qi).any(dim=1).cpu().numpy())[:8]
    assert torch.equal(jd.view(torch.int32), qd.view(torch.int32))
    assert index.last_join["queries"] == len(Y)
    return index.last_join


def test_the_slow_path_is_sound():
    from cilrs_mi355 import neighbours as NB
    Q, D, k = 2 * TQ, 64, 8
    assert Q >= NB.JOIN_MIN_Q
    X = KC.relu_rows(600, D, 11)
    Y = KC.relu_rows(Q, D, 12)
    # every row shifted by +30 (D = 512): norms about 1,500 times the distances, nothing can be certified
    X5, Y5 = KC.relu_rows(600, 512, 14) + 30, KC.relu_rows(Q, 512, 15) + 30
    assert not KJ.must_certify(X5, Y5[:64], k).any()
    last = _join_is_query(_index(X5), Y5, k)
    assert last["uncertified"] == Q, last
    # 40 near-copies of one row, that row among the queries: more near-ties than K_s
    rng = np.random.default_rng(13)
    Xc = X.copy()
    Xc[100:140] = Xc[100] + (1e-4 * rng.standard_normal((40, D))).astype(np.float32)
    Yc = Y.copy()
    Yc[5] = Xc[100]
    last = _join_is_query(_index(Xc), Yc, k)
    assert 0 < last["uncertified"] < Q, last
    # all rows equal
    last = _join_is_query(_index(np.tile(X[:1], (300, 1))), Y, k)
    assert last["uncertified"] > 0, last
    # N < K, and N - 1 < K with skip: the -1 / +inf fill comes from the certified path (a)
    small = _index(X[:5])
    last = _join_is_query(small, Y, k)
    assert last["uncertified"] == 0, last
    skip = torch.arange(Q) % 9                    # 5..8 are outside 0..N-1
    ji, jd = small.join(torch.from_numpy(Y).cuda(), 5, skip=skip)
    assert bool((ji[:, -1] == -1).eq(skip.cuda() < 5).all()) and bool(torch.isinf(jd[skip.cuda() < 5, -1]).all())
    _join_is_query(small, Y, 5, skip=skip)
    # one pool row with a NaN: max nx is not finite, every query falls back (include/cilrs_hip.h)
    Xn = X.copy()
    Xn[17, 3] = np.nan
    last = _join_is_query(_index(Xn), Y, k)
    assert last["uncertified"] == Q, last
    # a row with an entry whose square overflows, queried by itself (distance exactly 0)
    Xo = X.copy()
    Xo[33, 2] = 3e19
    Yo = Y.copy()
    Yo[7] = Xo[33]
    last = _join_is_query(_index(Xo), Yo, k)
    assert last["uncertified"] == Q, last
    # a NaN query beside finite ones: only that query falls back
    Yn = Y.copy()
    Yn[9, 0] = np.nan
    must = KJ.must_certify(X, Y, k)
    last = _join_is_query(_index(X), Yn, k)
    assert 1 <= last["uncertified"] <= 1 + int((~must).sum()), last
    # +inf distances: a query with an entry of 3e19 is at +inf from every row
    Yi = Y.copy()
    Yi[3, 1] = 3e19
    last = _join_is_query(_index(X), Yi, k)
    assert last["uncertified"] >= 1, last
    qi, qd = _index(X).join(torch.from_numpy(Yi).cuda(), k)
    assert bool(torch.isinf(qd[3]).all()) and qi[3].tolist() == list(range(k))


@pytest.mark.parametrize("metric", ["euclidean", "mahalanobis"])
def test_join_graph_and_bulk_calibration_are_query(metric):
    from cilrs_mi355 import neighbours as NB
    F, N, k = 512, 700, 8
    X = KC.relu_rows(N, F, 21)
    index = _index(X, metric)
    for Q in (NB.JOIN_MIN_Q - 1, NB.JOIN_MIN_Q, 2 * TQ + 3):
        Y, rows = TKN._queries(X, Q, 22 + Q)
        last = _join_is_query(index, Y, k)
        assert last["uncertified"] <= Q
        if metric == "euclidean":
            must = KJ.must_certify(X, Y, k)
            assert last["uncertified"] <= int((~must).sum()), (Q, last)
        _join_is_query(index, Y, k, skip=torch.from_numpy(rows))
    # raw pool rows whitened by the same kernel are at distance exactly 0 from their own row
    ji, jd = index.join(torch.from_numpy(X).cuda(), 1)
    assert torch.equal(ji[:, 0].cpu(), torch.arange(N)) and not jd.any()
    gi, gd = index.graph(k)
    qi, qd = index._query_rows(index.rows, k, torch.arange(N))
    assert torch.equal(gi, qi) and torch.equal(gd.view(torch.int32), qd.view(torch.int32))
    assert index.last_join["queries"] == N and not bool((gi == torch.arange(N).cuda()[:, None]).any())
    index.calibrate(k)
    slow = index.log[:index.log_count].clone()
    index.calibrate(k + 1)                        # another k starts the log again
    index.calibrate(k, bulk=True)
    assert index.log_count == N and torch.equal(index.log[:N].view(torch.int32), slow.view(torch.int32))
    index.calibrate(k, rows=[2, 5], bulk=True)
    assert index.log_count == N + 2
    for bad in (0, 17):
        with pytest.raises(ValueError, match="query"):
            index.join(torch.from_numpy(X).cuda(), bad)
        with pytest.raises(ValueError, match="1..16"):
            index.graph(bad)
    with pytest.raises(ValueError, match="1..16"):
        index.calibrate(17, bulk=True)
    index.calibrate(17)                           # the default path keeps its range


# ---- FramePool ---------------------------------------------------------------------------------------
class _Width(torch.nn.Module):
    """what FramePool asks of a model when rows come in through add_features"""

    def __init__(self, F):
        super().__init__()
        self.FEATURES = F
        self.p = torch.nn.Parameter(torch.zeros(1))


def _pool_of(X):
    from cilrs_mi355 import FramePool
    pool = FramePool(_Width(X.shape[1]).cuda(), len(X))
    return pool.add_features(torch.from_numpy(np.ascontiguousarray(X)).cuda())


def test_nearest_and_novel_rows():
    F, k = 64, 3
    drive, labelled = KC.relu_rows(400, F, 31), KC.relu_rows(500, F, 32)
    drive[::5] = labelled[:80]                    # every fifth frame of the drive is labelled already
    pool, index = _pool_of(drive), _index(labelled)
    idx, dist = pool.nearest(index, k)
    qi, qd = index.query(pool.features(), k)
    assert torch.equal(idx, qi) and torch.equal(dist.view(torch.int32), qd.view(torch.int32))
    assert torch.equal(idx[::5, 0].cpu(), torch.arange(80)) and not dist[::5, 0].any()
    # against a count over the device's own distances (cilrs_kcenter_cover of each labelled row)
    mind = torch.full((400,), float("inf"), dtype=torch.float32, device="cuda")
    TK._cover(pool.features(), 400, F, index.rows, 500, mind)
    torch.cuda.synchronize()
    assert torch.equal(dist[:, 0].view(torch.int32), mind.view(torch.int32))
    radius2 = float(np.median(mind.cpu().numpy().astype(np.float64)))
    want = np.flatnonzero(mind.cpu().numpy().astype(np.float64) > np.float64(np.float32(radius2)))
    got = pool.novel_rows(index, np.float32(radius2))
    assert np.array_equal(got.cpu().numpy(), want) and 0 < len(want) < 400 and not (want % 5 == 0).any()
    with pytest.raises(RuntimeError, match="features"):
        pool.nearest(_index(KC.relu_rows(50, 32, 1)))


def test_select_with_a_covered_index():
    from cilrs_mi355 import NeighbourIndex
    m, _orc = TM._pair()
    fd, _feats = TN._fitted_density()
    from cilrs_mi355 import FramePool
    F, k = 512, 12
    drive = torch.from_numpy(KC.relu_rows(330, F, 41)).cuda()
    C = torch.from_numpy(KC.relu_rows(300, F, 42)).cuda()
    pool = FramePool(m, 330).add_features(drive)
    for density in (fd, None):
        if density is None:
            ix = NeighbourIndex(C.clone())
        else:
            ix = NeighbourIndex(density.whiten(C).contiguous(), "mahalanobis", density._origin().clone(),
                                density.W.clone(), whitened=True)
        a = pool.select(k, density=density, covered=C)
        b = pool.select(k, density=density, covered_index=ix)
        assert np.array_equal(a.indices, b.indices) and _same_bits(a.radius, b.radius), density
        assert len(b.indices) == k and ix.last_join["queries"] == 330
    with pytest.raises(RuntimeError, match="euclidean"):
        pool.select(k, density=fd, covered_index=NeighbourIndex(C.clone()))
    mah = NeighbourIndex(fd.whiten(C).contiguous(), "mahalanobis", fd._origin().clone(), fd.W.clone())
    with pytest.raises(RuntimeError, match="mahalanobis"):
        pool.select(k, covered_index=mah)
    other = NeighbourIndex(fd.whiten(C).contiguous(), "mahalanobis", fd._origin().clone() + 1, fd.W.clone())
    with pytest.raises(RuntimeError, match="other tables"):
        pool.select(k, density=fd, covered_index=other)
    with pytest.raises(ValueError, match="first"):
        pool.select(k, first=3, covered_index=NeighbourIndex(C.clone()))


def test_select_covers_more_than_65536_rows():
    """the case covered= cannot be asked: a labelled set of 70,000 rows (F = 4, a cheap shape)"""
    M, N, k = 70000, 300, 6
    labelled, drive = KC.relu_rows(M, 4, 51), KC.relu_rows(N, 4, 52, scale=3.0)
    pool, ix = _pool_of(drive), _index(labelled)
    with pytest.raises(RuntimeError, match="65536"):
        pool.select(k, covered=torch.from_numpy(labelled).cuda())
    s = pool.select(k, covered_index=ix)
    assert len(s.indices) == k and (np.diff(s.radius) <= 0).all()
    # the first pick is the row farthest from the labelled set, by the device's own distances in halves
    mind = torch.full((N,), float("inf"), dtype=torch.float32, device="cuda")
    for lo in (0, 35000):
        TK._cover(pool.features(), N, 4, ix.rows[lo:lo + 35000], 35000, mind)
    torch.cuda.synchronize()
    assert s.indices[0] == int(mind.argmax()) and s.radius[0] == float(mind.max())


# ---- refusals ----------------------------------------------------------------------------------------
REFUSALS = {
    "null X": (dict(X=None), "NULL"),
    "null Y": (dict(Y=None), "NULL"),
    "null idx": (dict(null="idx"), "NULL"),
    "null dist": (dict(null="dist"), "NULL"),
    "null uncertified": (dict(null="unc"), "NULL"),
    "null n_uncertified": (dict(null="cnt"), "NULL"),
    "null scratch": (dict(null="scratch"), "scratch"),
    "N 0": (dict(N=0), "N ="),
    "N above 2^24": (dict(N=(1 << 24) + 1), "N ="),
    "D 0": (dict(D=0), "D ="),
    "D 6": (dict(D=6), "D ="),
    "D 2052": (dict(D=2052, ld=2052, ldq=2052), "D ="),
    "ld below D": (dict(ld=8), "ld ="),
    "ld 14": (dict(ld=14), "ld ="),
    "ldq below D": (dict(ldq=8), "ldq ="),
    "ldq 18": (dict(ldq=18), "ldq ="),
    "Q 0": (dict(Q=0), "Q ="),
    "Q 65537": (dict(Q=65537), "Q ="),
    "K 0": (dict(K=0), "K ="),
    "K 17": (dict(K=17), "K ="),
    "X off by 4 bytes": (dict(X_off=4), "aligned"),
    "Y off by 8 bytes": (dict(Y_off=8), "aligned"),
    "scratch off by 4 bytes": (dict(s_off=4), "aligned"),
    "scratch one byte short": (dict(short=1), "scratch"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_everything_untouched(name):
    kw, text = REFUSALS[name]
    L = _lib()
    N, Q, D, K = 40, 5, 12, 3
    if "X" not in _CACHE:
        _CACHE["X"] = (_dev_rows(KC.relu_rows(N, D, 1), 4), _dev_rows(KC.relu_rows(Q, D, 2), 4))
    X_d, Y_d = _CACHE["X"]
    out = _Out(N, Q, D, K, short=kw.get("short", 0))
    null = kw.get("null")

    def p(t, off=0):
        return None if t is None else TK._off(t, off)

    rc = L.lib().cilrs_knn_join(
        p(kw.get("X", X_d), kw.get("X_off", 0)), kw.get("ld", X_d.stride(0)), kw.get("N", N), kw.get("D", D),
        p(kw.get("Y", Y_d), kw.get("Y_off", 0)), kw.get("ldq", Y_d.stride(0)), kw.get("Q", Q), None,
        kw.get("K", K), None if null == "idx" else L.ptr(out.idx), None if null == "dist" else L.ptr(out.dist),
        None if null == "unc" else L.ptr(out.unc), None if null == "cnt" else L.ptr(out.cnt),
        None if null == "scratch" else p(out.scratch, kw.get("s_off", 0)), out.nbytes - kw.get("short", 0), _st())
    assert rc != 0 and text in _err(), (name, rc, _err())
    out.untouched()
    lib = L.lib()
    for args in ((0, 5, 12, 3), (40, 0, 12, 3), (40, 65537, 12, 3), (40, 5, 6, 3), (40, 5, 2052, 3),
                 (40, 5, 12, 0), (40, 5, 12, 17)):
        assert lib.cilrs_knn_join_scratch_bytes(*args) == 0, args
    assert lib.cilrs_knn_join_candidates(0) == 0 and lib.cilrs_knn_join_candidates(17) == 0


def test_scratch_stays_below_the_pool_at_the_flagship_size():
    lib = _lib().lib()
    assert 0 < lib.cilrs_knn_join_scratch_bytes(176256, 65536, 512, 16) <= 176256 * 512 * 4
    assert 0 < lib.cilrs_knn_join_scratch_bytes(176256, 64, 512, 16) <= 176256 * 512 * 4
