"""K nearest neighbours on the device (csrc/knn.hip: cilrs_knn; csrc/novelty.hip:
cilrs_feature_whiten; cilrs_net_knn, cilrs_mi355.neighbours.NeighbourIndex and
Predictor.predict_neighbours) against the definition of include/cilrs_hip.h ("Nearest neighbours").

Gates.  Op level, bit-exact: cilrs_kcenter_cover of each single query into a +inf mind gives the
device's own d(X_i, y_q); dist[q][j] must equal mind[idx[q][j]] bit for bit and (idx, dist) must equal
the first K entries of a numpy lexsort by (mind, i) with NaN and skipped rows removed (tests/_knn.py,
order).  Against float64: every returned distance within _kcenter.bound(D) relative of the float64
distance, and no row left out of a result closer in float64 than (1 - 2 bound) times the K-th
returned distance.  Both float64 gates leave out distances beyond FLT_MAX, where fp32 holds +inf.
Whitening: y against the float64 evaluation of the same rounded tables within
e_i = (i + 18) 2^-24 sum_j |W_ij||u_j| (test_novelty_gpu.py, docstring).

What the cases cross.  A chunk holds eight queries in LDS: Q = 1 and 8 stay inside one, 9 and 17
cross it.  The sweep runs at most 1,024 workgroups of 4 waves and a wave takes ROWS[D] rows at a time
(4 up to D = 512, 2 up to 1,024, else 1): one pass of the grid covers 4,096 * ROWS[D] rows, N = that
+ 5 makes some waves loop; N = 1 and 3 are below every K but 1 and 2.  K = 63 and 64 fill the lanes
of a wave's list.  The workgroups' lists of a query are folded in one launch up to 2,048 pairs, else
in two: N = 257 (65 workgroups) crosses that at K = 63, the looping N at K = 2 and above.  Outputs are pre-filled (idx -7, dist NaN) inside guard bands (tests/_guards.py),
the scratch is exactly cilrs_knn_scratch_bytes, the pad columns of X and Y hold NaN.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import _guards as G
import _kcenter as KC
import _knn as KN
import cilrs_oracle as O
import test_kcenter_gpu as TK
import test_mc_dropout_gpu as TM
import test_novelty_gpu as TN

pytestmark = pytest.mark.gpu

GRID_WAVES = TK.GRID_WAVES
FLT_MAX = float(np.finfo(np.float32).max)
KS = (1, 2, 63, 64)
_CACHE = {}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


_st, _err, _dev_rows = TK._st, TK._err, TK._dev_rows


class _Out:
    """guarded idx (-7) / dist (NaN) and an exactly sized scratch"""

    def __init__(self, N, Q, K, short=0, extra=0):
        self.nbytes = _lib().lib().cilrs_knn_scratch_bytes(N, Q, K)
        self.idx, c1 = G.guarded(Q * K, dtype=torch.int64, fill=-7, name="idx")
        self.dist, c2 = G.guarded(Q * K, name="dist")
        self.scratch, c3 = G.guarded(max(self.nbytes - short + extra, 1), dtype=torch.uint8, fill=0xA5,
                                     name="scratch")
        self.checks = (c1, c2, c3)
        self.Q, self.K = Q, K

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        assert bool((self.idx == -7).all()) and bool(torch.isnan(self.dist).all()) and \
            bool((self.scratch == 0xA5).all()), "a refused call wrote to its outputs"

    def host(self):
        return self.idx.view(self.Q, self.K).cpu().numpy(), self.dist.view(self.Q, self.K).cpu().numpy()


def _knn(X_d, N, D, Y_d, Q, K, skip=None):
    """one guarded call; returns (idx [Q][K], dist [Q][K]) on the host after every band was checked"""
    L = _lib()
    out = _Out(N, Q, K)
    skip_d = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.int64)).cuda()
    ins = G.Inputs(X=X_d, Y=Y_d, skip=skip_d)
    L.check(L.lib().cilrs_knn(L.ptr(X_d), X_d.stride(0), N, D, L.ptr(Y_d), Y_d.stride(0), Q,
                              L.ptr(skip_d), K, L.ptr(out.idx), L.ptr(out.dist), L.ptr(out.scratch),
                              out.nbytes, _st()))
    out.check()
    ins.check()
    return out.host()


def _device_distances(X_d, N, D, Y_d, Q):
    """mind [Q][N]: cilrs_kcenter_cover of each single query into a +inf mind.  The cover's minimum
    never takes a NaN, so the rows whose distance is NaN -- those that hold one: the queries are
    finite -- are marked here."""
    mind = torch.full((Q, N), float("inf"), dtype=torch.float32, device="cuda")
    for q in range(Q):
        TK._cover(X_d, N, D, Y_d[q:q + 1], 1, mind[q])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Y_d[:, :D]).all())
    mind = mind.cpu().numpy()
    mind[:, torch.isnan(X_d[:N, :D]).any(dim=1).cpu().numpy()] = np.nan
    return mind


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check(idx, dist, mind, d64, K, skip, D, what):
    """the gates of the docstring for one call; returns the largest share of the bound used"""
    Q, N = mind.shape
    b, share = KC.bound(D), 0.0
    for q in range(Q):
        sk = -1 if skip is None else int(skip[q])
        want_i, want_d = KN.order(mind[q], K, sk)
        assert np.array_equal(idx[q], want_i), (what, q, idx[q], want_i)
        assert _same_bits(dist[q], want_d), (what, q, dist[q], want_d)
        got = idx[q] >= 0
        assert _same_bits(dist[q][got], mind[q][idx[q][got]]), (what, q)
        assert np.isinf(dist[q][~got]).all() and (dist[q][~got] > 0).all()
        if d64 is None:
            continue
        ref = d64[q][idx[q][got]]
        fits = ref <= FLT_MAX * (1.0 - b)
        assert KC.close(dist[q][got][fits], ref[fits], b).all(), (what, q)
        pos = fits & (ref > 0)
        if pos.any():
            share = max(share, float((np.abs(dist[q][got][pos] - ref[pos]) / (b * ref[pos])).max()))
        if got.all() and np.isfinite(dist[q][-1]):
            out = np.ones(N, dtype=bool)
            out[idx[q]] = False
            if 0 <= sk < N:
                out[sk] = False
            out &= ~np.isnan(d64[q])
            assert (d64[q][out] >= (1.0 - 2.0 * b) * float(dist[q][-1])).all(), \
                f"{what}: query {q} leaves out a row nearer than its K-th neighbour"
    return share


def _float64(X, Y):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([KC.dist(X, y) for y in Y])


def _queries(X, Q, seed):
    """relu-shaped queries; every third one is a row of the pool (distance 0, leave-one-out)"""
    N, D = X.shape
    Y = KC.relu_rows(Q, D, seed)
    rows = np.full(Q, -1, dtype=np.int64)
    for q in range(0, Q, 3):
        rows[q] = (q * 7919 + N // 2) % N
        Y[q] = X[rows[q]]
    return Y, rows


# ---- shapes ------------------------------------------------------------------------------------------
def _pass_rows(D):
    return GRID_WAVES * TK.rows_per_wave(D) + 5


SHAPES = [(D, N) for D in (4, 256, 260, 512, 1024, 2048) for N in (1, 3, "pass")]


@pytest.mark.parametrize("D,N", SHAPES, ids=[f"d{D}_n{N}" for D, N in SHAPES])
def test_every_variant_against_the_cover_kernel_and_float64(D, N):
    loops = N == "pass"
    N = _pass_rows(D) if loops else N
    Q = 9 if loops else 17
    X = KC.relu_rows(N, D, 3 * D + N)
    Y, own = _queries(X, Q, 50 + D)
    d64 = _float64(X, Y)
    worst = 0.0
    for pad in (0, 4):
        X_d, Y_d = _dev_rows(X, pad), _dev_rows(Y, 4 - pad)
        mind = _device_distances(X_d, N, D, Y_d, Q)
        for K in KS:
            skip = None if K in (1, 63) else own
            idx, dist = _knn(X_d, N, D, Y_d, Q, K, skip)
            worst = max(worst, _check(idx, dist, mind, d64, K, skip, D, f"N={N} D={D} pad={pad} K={K}"))
            if skip is None:                                 # (relu rows at D = 4 repeat: any copy)
                assert not dist[::3, 0].any() and np.array_equal(X[idx[::3, 0]], Y[::3])
            if N < K:
                assert (idx[:, N:] == -1).all()
    print(f"knn N={N} D={D}: largest share of the bound {worst:.3g}")


@pytest.mark.parametrize("Q", [1, 8, 9, 17])
def test_query_counts_across_the_chunk_of_eight(Q):
    N, D = 257, 512
    X = KC.relu_rows(N, D, 21)
    Y, own = _queries(X, Q, 22 + Q)
    X_d, Y_d = _dev_rows(X, 4), _dev_rows(Y, 0)
    mind, d64 = _device_distances(X_d, N, D, Y_d, Q), _float64(X, Y)
    for K in KS:
        idx, dist = _knn(X_d, N, D, Y_d, Q, K)
        _check(idx, dist, mind, d64, K, None, D, f"Q={Q} K={K}")


def test_integer_rows_with_duplicates_tie_across_workgroups():
    N, D, Q = GRID_WAVES * 4 + 5, 4, 17
    X = TK._int_rows(N, D, 7)                                # 8^4 distinct rows at the most: ties
    Y = np.concatenate([X[[0, N - 1, 4096, 9000]], TK._int_rows(Q - 4, D, 8)])
    X_d, Y_d = _dev_rows(X, 0), _dev_rows(Y, 4)
    mind = _device_distances(X_d, N, D, Y_d, Q)
    d64 = _float64(X, Y)
    assert np.array_equal(mind.astype(np.float64), d64), "integer rows: every fp32 sum is exact"
    skip = np.array([0, N - 1, 5, -1, N, 1 << 40, -(1 << 40)] + [3] * (Q - 7), dtype=np.int64)
    for K in KS:
        for sk in (None, skip):
            idx, dist = _knn(X_d, N, D, Y_d, Q, K, sk)
            want_i, want_d = KN.knn(X, Y, K, sk)             # the float64 definition, bit for bit
            assert np.array_equal(idx, want_i) and np.array_equal(dist.astype(np.float64), want_d)
            _check(idx, dist, mind, d64, K, sk, D, f"integer rows K={K}")
    idx, dist = _knn(X_d, N, D, Y_d, Q, 64)
    ties = sum(len(set(d.tolist())) < 64 for d in dist)
    assert ties == Q and (np.diff(idx[0][dist[0] == dist[0][0]]) > 0).all()
    assert len({int(i) // 16 for i in idx[0]}) > 8, "the ties of query 0 come from many workgroups"


def test_skip_forms():
    N, D, Q, K = 257, 12, 9, 5
    X = KC.relu_rows(N, D, 31)
    Y = X[np.arange(Q) * 28].copy()                          # every query is a pool row
    own = np.arange(Q, dtype=np.int64) * 28
    X_d, Y_d = _dev_rows(X, 4), _dev_rows(Y, 4)
    mind, d64 = _device_distances(X_d, N, D, Y_d, Q), _float64(X, Y)
    plain = _knn(X_d, N, D, Y_d, Q, K)
    _check(*plain, mind, d64, K, None, D, "no skip")
    assert np.array_equal(plain[0][:, 0], own) and not plain[1][:, 0].any()
    for name, skip in (("-1", np.full(Q, -1)), (">= N", np.arange(Q) + N), ("huge", np.full(Q, 1 << 33))):
        got = _knn(X_d, N, D, Y_d, Q, K, skip)
        assert np.array_equal(got[0], plain[0]) and _same_bits(got[1], plain[1]), name
    loo = _knn(X_d, N, D, Y_d, Q, K, own)
    _check(*loo, mind, d64, K, own, D, "leave one out")
    assert not (loo[0] == own[:, None]).any()
    assert np.array_equal(loo[0][:, :K - 1], plain[0][:, 1:]) and (loo[1][:, 0] > 0).all()


def test_nan_rows_and_infinite_distances():
    N, D, Q, K = 300, 260, 3, 64
    X = KC.relu_rows(N, D, 41)
    X[5] = np.nan
    X[17, 259] = np.nan                                      # one NaN column, the last of the row
    X[100:110] = 0.9 * FLT_MAX                               # d = +inf: an ordinary value
    X[250:] = np.nan
    Y = KC.relu_rows(Q, D, 42)
    X_d, Y_d = _dev_rows(X, 4), _dev_rows(Y, 0)
    mind, d64 = _device_distances(X_d, N, D, Y_d, Q), _float64(X, Y)
    assert np.isposinf(mind[:, 100:110]).all() and np.isnan(d64[:, [5, 17]]).all()
    live = N - 52 - 10
    for K in (64, 2):
        idx, dist = _knn(X_d, N, D, Y_d, Q, K)
        _check(idx, dist, mind, d64, K, None, D, f"NaN rows K={K}")
        assert not np.isin(idx, [5, 17] + list(range(250, N))).any()
    # K reaches into the infinite rows when few finite ones are left
    few = np.concatenate([X[100:110], X[:3], X[250:260]])    # 10 at +inf, 3 finite, 10 NaN
    f_d = _dev_rows(few, 0)
    m2 = _device_distances(f_d, 23, D, Y_d, Q)
    idx, dist = _knn(f_d, 23, D, Y_d, Q, 16)
    _check(idx, dist, m2, None, 16, None, D, "infinite rows")
    assert (np.sort(idx[:, :3], axis=1) == [10, 11, 12]).all() and np.isfinite(dist[:, :3]).all()
    assert (idx[:, 3:13] == np.arange(10)).all() and np.isposinf(dist[:, 3:13]).all()
    assert (idx[:, 13:] == -1).all() and np.isposinf(dist[:, 13:]).all()
    # every row NaN: every slot -1 / +inf
    nan_d = torch.full((37, D), float("nan"), device="cuda")
    idx, dist = _knn(nan_d, 37, D, Y_d, Q, 8)
    assert (idx == -1).all() and np.isposinf(dist).all()
    assert live > 64


def test_repeatability():
    N, D, Q = 2 * GRID_WAVES + 3, 1024, 17
    X = KC.relu_rows(N, D, 61)
    Y, _own = _queries(X, Q, 62)
    X_d, Y_d = _dev_rows(X, 0), _dev_rows(Y, 4)
    i64, d64 = _knn(X_d, N, D, Y_d, Q, 64)
    again = _knn(X_d, N, D, Y_d, Q, 64)
    assert np.array_equal(again[0], i64) and _same_bits(again[1], d64)
    i8, d8 = _knn(X_d, N, D, Y_d, Q, 8)                      # K = 8 is the prefix of K = 64
    assert np.array_equal(i8, i64[:, :8]) and _same_bits(d8, d64[:, :8])
    for q in (0, 7, 8, 16):                                  # a query of a batch is the query alone
        ia, da = _knn(X_d, N, D, Y_d[q:q + 1], 1, 64)
        assert np.array_equal(ia[0], i64[q]) and _same_bits(da[0], d64[q])
    # rows in another place of the grid: the first 1,000 rows alone against the rows of 0..999 in
    # the full result
    ip, dp = _knn(X_d, 1000, D, Y_d, Q, 64)
    for q in range(Q):
        keep = i64[q] < 1000
        n = int(keep.sum())
        assert np.array_equal(ip[q][:n], i64[q][keep]) and _same_bits(dp[q][:n], d64[q][keep])


def test_scratch_size_query():
    lib = _lib().lib()
    assert lib.cilrs_knn_scratch_bytes(1, 1, 1) > 0
    for N, Q, K in ((3, 1, 64), (4096, 8, 8), (4097, 9, 64), (176256, 65536, 64), (1 << 24, 1, 1)):
        n = lib.cilrs_knn_scratch_bytes(N, Q, K)
        assert 0 < n <= (1024 + 32) * 8 * 64 * 8 and n % 8 == 0
        assert n == lib.cilrs_knn_scratch_bytes(N, min(Q, 8), K)
    for N, Q, K in ((0, 1, 1), ((1 << 24) + 1, 1, 1), (5, 0, 1), (5, 65537, 1), (5, 1, 0), (5, 1, 65),
                    (-1, 1, 1), (5, -1, 1), (5, 1, -1)):
        assert lib.cilrs_knn_scratch_bytes(N, Q, K) == 0


# ---- refusals ----------------------------------------------------------------------------------------
def _refusal_args():
    N, D, Q = 5, 12, 3
    X_d = _dev_rows(KC.relu_rows(N, D, 1), 4)
    Y_d = _dev_rows(KC.relu_rows(Q, D, 2), 4)
    return dict(X=X_d, ld=X_d.stride(0), N=N, D=D, Y=Y_d, ldq=Y_d.stride(0), Q=Q, K=2)


REFUSALS = {
    "null X": (dict(X=None), "NULL"),
    "null Y": (dict(Y=None), "NULL"),
    "null idx": (dict(null="idx"), "NULL"),
    "null dist": (dict(null="dist"), "NULL"),
    "N 0": (dict(N=0), "N ="),
    "N above 2^24": (dict(N=(1 << 24) + 1), "N ="),
    "D 0": (dict(D=0), "D ="),
    "D 6": (dict(D=6, ld=8, ldq=8), "D ="),
    "D 2052": (dict(D=2052, ld=2052, ldq=2052), "D ="),
    "ld below D": (dict(ld=8), "ld ="),
    "ld 14": (dict(ld=14), "ld ="),
    "ldq below D": (dict(ldq=8), "ldq ="),
    "ldq 18": (dict(ldq=18), "ldq ="),
    "X off by 4 bytes": (dict(X_off=4), "aligned"),
    "Y off by 8 bytes": (dict(Y_off=8), "aligned"),
    "Q 0": (dict(Q=0), "Q ="),
    "Q 65537": (dict(Q=65537), "Q ="),
    "K 0": (dict(K=0), "K ="),
    "K 65": (dict(K=65), "K ="),
    "null scratch": (dict(null="scratch"), "scratch"),
    "scratch one byte short": (dict(short=1), "scratch"),
    "scratch off by 8 bytes": (dict(scratch_off=8), "aligned"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_launch_nothing(case):
    change, text = REFUSALS[case]
    a = _refusal_args()
    a.update(change)
    L = _lib()
    null, off = a.get("null"), a.get("scratch_off", 0)
    out = _Out(5, 3, 2, short=a.get("short", 0), extra=16 if off else 0)
    rc = L.lib().cilrs_knn(
        None if a["X"] is None else TK._off(a["X"], a.get("X_off", 0)), a["ld"], a["N"], a["D"],
        None if a["Y"] is None else TK._off(a["Y"], a.get("Y_off", 0)), a["ldq"], a["Q"], None, a["K"],
        None if null == "idx" else L.ptr(out.idx), None if null == "dist" else L.ptr(out.dist),
        None if null == "scratch" else TK._off(out.scratch, off), out.nbytes - a.get("short", 0), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    out.untouched()


# ---- whitening -----------------------------------------------------------------------------------------
def _whiten(feat_d, B, F, origin_d, W_d, short=0, null=None):
    L = _lib()
    n = L.lib().cilrs_feature_whiten_scratch_floats(F, B)
    assert n == B * F
    y, c1 = G.guarded(B * F, name="y")
    scratch, c2 = G.guarded(max(n - short, 1), name="scratch")
    ins = G.Inputs(features=feat_d, origin=origin_d)
    rc = L.lib().cilrs_feature_whiten(
        L.ptr(feat_d), feat_d.stride(0), B, F, None if null == "origin" else L.ptr(origin_d),
        None if null == "W" else L.ptr(W_d), None if null == "y" else L.ptr(y),
        None if null == "scratch" else L.ptr(scratch), n - short, _st())
    c1()
    c2()
    ins.check()
    return rc, y.view(B, F), scratch


@pytest.mark.parametrize("F", [512, 2048])
def test_whiten_against_float64_of_the_same_tables(F):
    import _novelty as N
    import test_novelty_gpu as TN
    mean32, W32, mean_d, W_d = TN._tables(F, 4)              # the device W holds NaN where j > i
    origin, origin_d = mean32[1], mean_d[1].contiguous()
    worst = 0.0
    for B, pad in ((1, 0), (5, 128), (33, 4), (203, 0)):     # above 64 frames the launch splits them
        v, _cmd = N.relu_features(B, F, 4, 70 + B)
        feat_d = TM._pooled_dev(torch.from_numpy(v), F + pad)
        rc, y, _s = _whiten(feat_d, B, F, origin_d, W_d)
        assert rc == 0, _err()
        G.all_finite(y, "y")
        ref, mag = KN.whiten64(v, origin, W32)
        e = (np.arange(F) + 18) * 2.0 ** -24 * mag
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(e, 1e-300)).max()))
        assert (err <= e).all(), (F, B)
        rc, y2, _s = _whiten(feat_d, B, F, origin_d, W_d)    # two runs are bit-identical
        assert torch.equal(y2, y)
        for b in sorted({0, B // 2, B - 1}):                 # row b of a batch is the row alone
            rc, alone, _s = _whiten(feat_d[b:b + 1], 1, F, origin_d, W_d)
            assert rc == 0 and torch.equal(alone[0], y[b]), (F, B, b)
    print(f"whiten F={F}: largest share of the bound {worst:.3g}")


def test_whiten_refusals_launch_nothing():
    import test_novelty_gpu as TN
    F, B = 512, 3
    _m, _w, mean_d, W_d = TN._tables(F, 4)
    feat_d = TM._pooled_dev(torch.from_numpy(KC.relu_rows(B, F, 1)), F)
    origin_d = mean_d[0].contiguous()
    L = _lib()
    for kw, text in ((dict(null="origin"), "NULL"), (dict(null="W"), "NULL"), (dict(null="y"), "NULL"),
                     (dict(null="scratch"), "scratch"), (dict(short=1), "scratch")):
        rc, y, scratch = _whiten(feat_d, B, F, origin_d, W_d, **kw)
        assert rc != 0 and text in _err(), (kw, _err())
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(scratch).all())
    y, check = G.guarded(B * F, name="y")
    s, check_s = G.guarded(B * F, name="scratch")
    for args, text in (((feat_d, F, 0, F), "batch"), ((feat_d, F, 65537, F), "batch"),
                       ((feat_d, F, B, 500), "feature width"), ((feat_d, F, B, 1024), "feature width"),
                       ((feat_d, F - 1, B, F), "ld"), ((None, F, B, F), "NULL")):
        f, ld, b, width = args
        rc = L.lib().cilrs_feature_whiten(L.ptr(f), ld, b, width, L.ptr(origin_d), L.ptr(W_d), L.ptr(y),
                                          L.ptr(s), B * F, _st())
        assert rc != 0 and text in _err(), (args[1:], _err())
    rc = L.lib().cilrs_feature_whiten(L.ptr(feat_d), F, B, F, L.ptr(origin_d), TK._off(W_d, 4), L.ptr(y),
                                      L.ptr(s), B * F, _st())
    assert rc != 0 and "aligned" in _err()
    check()
    check_s()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(s).all())
    lib = L.lib()
    for F_, B_ in ((500, 3), (512, 0), (512, -1), (2048, 65537)):
        assert lib.cilrs_feature_whiten_scratch_floats(F_, B_) == 0


# ---- plan level --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TN.PLAN_CASES))
def test_plan_level_after_each_eval_realisation(name):
    """cilrs_net_knn takes the tick's features exactly as the other plan-level entries do:
    `combined`, or after the persistent launch the cell-order average of the last feature map.  Its
    (idx, dist) equal, bit for bit, cilrs_knn of those features uploaded as queries -- after
    cilrs_feature_whiten of them when tables are given."""
    B, H, W, fwd, _source_name = TN.PLAN_CASES[name]
    m, _orc = TM._models50() if name == "resnet50" else TM._pair()
    F, NC = (2048, 4) if name == "resnet50" else (512, 4)
    N, K = 40, 8
    eng = m.engine()
    _img, spd, cmd, _t, u8 = O.synthetic_batch(B, seed=77, h=H, w=W)
    u8_d, spd_d, cmd_d = torch.from_numpy(u8).cuda(), spd.cuda(), cmd.cuda()
    ctrl, ps = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    pl = eng.last_plan
    eng.check_status()
    before = (ctrl.clone(), ps.clone())
    v = np.ascontiguousarray(TN._plan_features32(pl, name == "persistent"), dtype=np.float32)
    assert v.shape == (B, F) and np.isfinite(v).all()
    v_d = _dev_rows(v, 0)
    _mean32, _W32, mean_d, W_d = TN._tables(F, NC)
    origin_d = mean_d[1].contiguous()
    L = _lib()
    need = L.lib().cilrs_net_knn_scratch_bytes(F, B, N, K)
    assert need == 2 * B * F * 4 + L.lib().cilrs_knn_scratch_bytes(N, B, K)

    def net_knn(X_d, origin, Wt):
        out = _Out(N, B, K)
        out.scratch, c = G.guarded(need, dtype=torch.uint8, fill=0xA5, name="scratch")
        out.checks = out.checks[:2] + (c,)
        ins = G.Inputs(X=X_d)
        L.check(L.lib().cilrs_net_knn(pl.handle, C.byref(pl.bufs), L.ptr(X_d), X_d.stride(0), N,
                                      L.ptr(origin), L.ptr(Wt), K, L.ptr(out.idx), L.ptr(out.dist),
                                      L.ptr(out.scratch), need, _st()))
        out.check()
        ins.check()
        return out.host()

    # origin = W = NULL: the features themselves are the queries
    X_d = _dev_rows(KC.relu_rows(N, F, 31, scale=float(v.max())), 4)
    idx, dist = net_knn(X_d, None, None)
    want_i, want_d = _knn(X_d, N, F, v_d, B, K)
    assert np.array_equal(idx, want_i) and _same_bits(dist, want_d), name
    assert (idx >= 0).all() and np.isfinite(dist).all()
    # with tables: cilrs_feature_whiten of the same features, then cilrs_knn
    rc, y_d, _s = _whiten(v_d, B, F, origin_d, W_d)
    assert rc == 0, _err()
    Xw_d = _dev_rows(KC.relu_rows(N, F, 32, scale=float(y_d.abs().max())), 0)
    idx, dist = net_knn(Xw_d, origin_d, W_d)
    want_i, want_d = _knn(Xw_d, N, F, y_d, B, K)
    assert np.array_equal(idx, want_i) and _same_bits(dist, want_d), name
    assert (idx >= 0).all() and np.isfinite(dist).all()
    assert pl.status.tolist()[0] == 0
    # the forward's own outputs: untouched, and the same from the next forward
    assert torch.equal(ctrl, before[0]) and torch.equal(ps, before[1])
    ctrl2, ps2 = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    assert torch.equal(ctrl2, before[0]) and torch.equal(ps2, before[1])


# ---- end to end --------------------------------------------------------------------------------------
POOL_BATCHES = (3, 5, 3, 5, 5, 3)


def _pool():
    """24 frames at 40x120 through FramePool.add, as test_kcenter_gpu.py's end-to-end case"""
    if "pool" not in _CACHE:
        from cilrs_mi355 import FramePool
        m, _orc = TM._pair()
        pool = FramePool(m, 24)
        batches = []
        for i, B in enumerate(POOL_BATCHES):
            img, spd, cmd, _t, u8 = O.synthetic_batch(B, seed=900 + i, h=40, w=120)
            pool.add(img.cuda(), spd.cuda(), cmd.cuda())
            batches.append((img, spd, cmd, u8))
        _CACHE["pool"] = (m, pool, batches)
    return _CACHE["pool"]


@pytest.mark.parametrize("metric", ["euclidean", "mahalanobis"])
def test_end_to_end_predict_neighbours(metric):
    import test_novelty_gpu as TN
    from cilrs_mi355 import NeighbourIndex
    from cilrs_mi355.predict import Predictor, SPEED_NORM_FACTOR
    m, pool, batches = _pool()
    fd, _feats = TN._fitted_density()                        # fitted on 40 other frames
    F, k = 512, 8
    index = pool.index(density=fd if metric == "mahalanobis" else None)
    assert isinstance(index, NeighbourIndex) and index.metric == metric and len(index) == 24
    assert index.rows.is_cuda and tuple(index.rows.shape) == (24, F)
    # the key of the weights the rows came from: the fit's with a density (the model's key moves on
    # whenever something may have changed the weights, so the two need not be equal), else the pool's
    assert index.weights_key == (fd.fit_weights_key if metric == "mahalanobis" else pool.weights_key) != 0
    feats = pool.features()
    if metric == "mahalanobis":
        k0 = int(np.flatnonzero(fd.present)[0])
        ref, mag = KN.whiten64(feats.cpu().numpy(), fd.mean.cpu().numpy()[k0], fd.W.cpu().numpy())
        err = np.abs(index.rows.cpu().numpy().astype(np.float64) - ref)
        assert (err <= (np.arange(F) + 18) * 2.0 ** -24 * mag).all()
        assert torch.equal(index.whiten(feats), index.rows)  # in chunks or at once: the same rows
    else:
        assert torch.equal(index.rows, feats) and index.rows.data_ptr() != feats.data_ptr()
    # every pool row finds itself first, at distance exactly 0, in both metrics
    qi, qd = index.query(feats, k)
    torch.cuda.synchronize()
    assert torch.equal(qi[:, 0].cpu(), torch.arange(24)) and not qd[:, 0].any()
    assert bool((qd[:, 1] > 0).all())
    rows64 = index.rows.cpu().numpy()
    want_i, want_d = KN.knn(rows64, rows64, k)
    assert KC.close(qd.cpu().numpy(), want_d, KC.bound(F)).all()
    # the per-layer predictor's features equal the pool's bit for bit
    preds = {B: Predictor(m, batch=B, height=40, width=120, persistent=False) for B in (3, 5)}
    b0 = 0
    for img, spd, cmd, u8 in batches:
        B = len(cmd)
        kmh = (spd.double() * SPEED_NORM_FACTOR).numpy()
        controls, pspeed, idx, dist = preds[B].predict_neighbours(u8, kmh, cmd.numpy(), index, k=k)
        assert idx.dtype == np.int64 and dist.dtype == np.float32 and idx.shape == dist.shape == (B, k)
        assert controls.dtype == pspeed.dtype == np.float32 and controls.shape == (B, 3)
        assert np.array_equal(idx[:, 0], np.arange(b0, b0 + B)), (idx[:, 0], b0)
        assert (dist[:, 0] == 0.0).all(), dist[:, 0]
        assert np.array_equal(idx, qi[b0:b0 + B].cpu().numpy())
        assert _same_bits(dist, qd[b0:b0 + B].cpu().numpy())
        point = preds[B].predict_batch(u8, kmh, cmd.numpy())
        assert np.array_equal(controls, point[:, :3]) and np.array_equal(pspeed, point[:, 3])
        b0 += B
    # the persistent single-frame predictor rounds its features differently: the row itself is
    # still the nearest by orders of magnitude
    one = Predictor(m, batch=1, height=40, width=120)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for b, (bi, r) in ((4, (1, 1)), (23, (5, 2))):
            img, spd, cmd, u8 = batches[bi]
            kmh = [float(spd[r]) * SPEED_NORM_FACTOR]
            controls, pspeed, idx, dist = one.predict_neighbours(u8[r:r + 1], kmh, [int(cmd[r])], index, k=k)
            print(f"{metric}, persistent={one.persistent}: frame {b} -> dist[0, 0] = {dist[0, 0]:.6g}, "
                  f"dist[0, 1] = {dist[0, 1]:.6g}")
            assert idx[0, 0] == b
            point = one.predict_batch(u8[r:r + 1], kmh, [int(cmd[r])])
            assert np.array_equal(controls, point[:, :3]) and np.array_equal(pspeed, point[:, 3])
        tick, ti, td = one.predict_controls_neighbours(u8[r], kmh[0], int(cmd[r]), index, k=3)
    assert len(tick) == 4 and ti.shape == td.shape == (3,) and np.array_equal(ti, idx[0, :3])
    # leave-one-out calibration never returns a row as its own neighbour
    loo_i, loo_d = index._query_rows(index.rows, 3, torch.arange(24))
    torch.cuda.synchronize()
    assert not (loo_i.cpu() == torch.arange(24)[:, None]).any()
    assert torch.equal(loo_i.cpu()[:, :2], qi.cpu()[:, 1:3])
    index.calibrate(3)
    s = index.calibration_scores()
    assert s.shape == (24,) and (s > 0).all() and np.array_equal(s, np.sort(loo_d[:, 2].cpu().numpy()))
    index.calibrate(3, rows=[2, 5])
    assert index.log_count == 26 and index.percentile(0.0) == 0.0 and index.percentile(np.inf) == 100.0


def test_predictor_and_plan_refusals(tmp_path):
    import test_novelty_gpu as TN
    from cilrs_mi355 import NeighbourIndex
    from cilrs_mi355.predict import Predictor
    m, pool, batches = _pool()
    fd, _feats = TN._fitted_density()
    index = pool.index(density=fd)
    u8 = batches[0][3]
    with pytest.raises(RuntimeError, match="fp32 predictors only"):
        Predictor(m, batch=3, height=40, width=120, half=True).predict_neighbours(
            u8, [10.0, 20.0, 30.0], [0, 1, 2], index)
    m50, _o = TM._models50()
    with pytest.raises(RuntimeError, match="features"):
        Predictor(m50, batch=1, height=40, width=120).predict_neighbours(u8[:1], [10.0], [0], index)
    pred = Predictor(m, batch=3, height=40, width=120, persistent=False)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must be"):
            pred.predict_neighbours(u8, [10.0, 20.0, 30.0], [0, 1, 2], index, k=k)
    other = NeighbourIndex(index.rows, "mahalanobis", index.origin, index.W, commands=5)
    with pytest.raises(RuntimeError, match="commands"):
        pred.predict_neighbours(u8, [10.0, 20.0, 30.0], [0, 1, 2], other)
    with pytest.raises(RuntimeError, match="single-frame"):
        pred.predict_controls_neighbours(u8[0], 30.0, 2, index)
    # plan level: no forward yet, a train-mode forward last, NULL tensors, a short scratch
    L = _lib()
    tm = TM._train_model()
    eng = tm.engine()
    img, spd, cmd, _t, _u8 = O.synthetic_batch(3, seed=5, h=40, w=120)
    K = 4
    need = L.lib().cilrs_net_knn_scratch_bytes(512, 3, 24, K)
    assert need == 2 * 3 * 512 * 4 + L.lib().cilrs_knn_scratch_bytes(24, 3, K)
    assert L.lib().cilrs_net_knn_scratch_bytes(500, 3, 24, K) == 0
    assert L.lib().cilrs_net_knn_scratch_bytes(512, 3, 24, 65) == 0

    def call(pl, out, rows=index.rows, origin=index.origin, W=index.W, short=0, null=None):
        return L.lib().cilrs_net_knn(
            pl.handle, C.byref(pl.bufs), L.ptr(rows), 512, 24, L.ptr(origin), L.ptr(W), K,
            None if null == "idx" else L.ptr(out.idx), None if null == "dist" else L.ptr(out.dist),
            L.ptr(out.scratch), need - short, _st())

    def plan_out(short=0):
        out = _Out(24, 3, K)
        out.scratch, c = G.guarded(need - short, dtype=torch.uint8, fill=0xA5, name="scratch")
        out.checks = out.checks[:2] + (c,)
        return out

    out = plan_out()
    assert call(eng.plan(3, 40, 120, lane=3), out) != 0 and "no forward" in _err()
    out.untouched()
    _c, _s, pl = eng.run_forward(img.cuda(), spd.cuda(), cmd.cuda(), True, 0.5, 1)
    torch.cuda.synchronize()
    assert call(pl, out) != 0 and "train mode" in _err()
    out.untouched()
    eng.run_forward(img.cuda(), spd.cuda(), cmd.cuda(), False, 0.0, 0)
    torch.cuda.synchronize()
    for kw, text in ((dict(rows=None), "NULL"), (dict(null="idx"), "NULL"), (dict(null="dist"), "NULL"),
                     (dict(origin=None), "go together"), (dict(W=None), "go together")):
        assert call(pl, out, **kw) != 0 and text in _err(), (kw, _err())
        out.untouched()
    short = plan_out(short=1)
    assert call(pl, short, short=1) != 0 and "scratch" in _err()
    short.untouched()
    # ... and the valid calls on the eval forward go through, in both metrics, inside the guards
    assert call(pl, out) == 0, _err()
    out.check()
    idx, dist = out.host()
    feats = eng.plan_features(pl).clone()
    want = index.query(feats, K)
    assert np.array_equal(idx, want[0].cpu().numpy()) and _same_bits(dist, want[1].cpu().numpy())
    out = plan_out()
    euc = pool.index()
    assert call(pl, out, rows=euc.rows, origin=None, W=None) == 0, _err()
    out.check()
    idx, dist = out.host()
    want = euc.query(feats, K)
    assert np.array_equal(idx, want[0].cpu().numpy()) and _same_bits(dist, want[1].cpu().numpy())
    # save / load on the device reproduces query exactly
    path = tmp_path / "index.pth"
    index.save(path)
    back = NeighbourIndex.load(path, device="cuda")
    a, b = index.query(feats, K), back.query(feats, K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and back.metric == "mahalanobis"
