"""K-means on the device (csrc/kmeans.hip: cilrs_kmeans_assign / _update / _lloyd,
cilrs_mi355.cluster) against the float64 definition and the walking checker of tests/_kmeans.py.

Gates: tests/_kmeans.py (docstring).  A distance is within KC.bound(D) of float64; labels are judged
on the device's own sequence, so a near-tie cannot make a test flaky; counts and changed are exact;
centres are the rounded float64 means to one fp32 ulp, bit for bit on integer rows; the assignment
equals cilrs_knn with X = C, Y = the rows, K = 1 bit for bit.

What the cases cross.  The assign kernel stages CHUNK[D] = 128 / 64 / 32 / 16 centres in LDS (128 KiB)
at D <= 256 / 512 / 1,024 / 2,048 and takes them in groups of 16 / ROWS[D] per butterfly, ROWS[D] =
4 / 4 / 2 / 1 rows per wave: K runs over 1, the eight of the old staging +- 1, CHUNK - 1, CHUNK,
CHUNK + 1 and two chunks and a tail.  A workgroup has 16 waves (8 above D = 512) and the grid at most
one workgroup per CU: N = 1, 2, 5, 9 leave a wave's batch partly filled, N = 257 and 1,030 take
several workgroups with a partial last batch, and the GRID_CASES hold more rows than one pass of a
256-CU grid.  The sums cut the rows into blocks of 256: N = 1,030 is five blocks with a tail.
Outputs sit NaN- / -7-filled inside guard bands (tests/_guards.py), the scratch is exactly
cilrs_kmeans_scratch_bytes, the pad columns of X and C hold NaN: they must not be read, and C's must
not be written.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _guards as G
import _kcenter as KC
import _kmeans as KM
import test_mc_dropout_gpu as TM

pytestmark = pytest.mark.gpu

CHUNK = {4: 128, 12: 128, 260: 64, 512: 64, 1024: 32, 2048: 16}
KS = {D: sorted({1, 7, 8, 9, c - 1, c, c + 1, 2 * c + 2}) for D, c in CHUNK.items()}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    msg = _lib().lib().cilrs_last_error()
    return msg.decode() if msg else ""


def _dev_rows(X, pad):
    return TM._pooled_dev(torch.from_numpy(np.ascontiguousarray(X)), X.shape[1] + pad)


class _Out:
    """guarded label / dist / counts / inertia / changed and an exactly sized scratch"""

    def __init__(self, N, D, K, iters=0, label0=None, short=0, extra=0):
        self.nbytes = _lib().lib().cilrs_kmeans_scratch_bytes(N, D, K)
        self.label, c1 = G.guarded(N, dtype=torch.int32, fill=-7, name="label")
        if label0 is not None:
            self.label.copy_(torch.from_numpy(np.asarray(label0, dtype=np.int32)))
        self.dist, c2 = G.guarded(N, name="dist")
        self.counts, c3 = G.guarded(K, dtype=torch.int64, fill=-7, name="counts")
        self.inertia, c4 = G.guarded(iters + 1, dtype=torch.float64, name="inertia")
        self.changed, c5 = G.guarded(iters + 1, dtype=torch.int64, fill=-7, name="changed")
        self.scratch, c6 = G.guarded(max(self.nbytes - short + extra, 1), dtype=torch.uint8, fill=0xA5,
                                     name="scratch")
        self.checks = (c1, c2, c3, c4, c5, c6)

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        assert bool((self.label == -7).all()) and bool(torch.isnan(self.dist).all()) and \
            bool((self.counts == -7).all()) and bool(torch.isnan(self.inertia).all()) and \
            bool((self.changed == -7).all()) and bool((self.scratch == 0xA5).all()), \
            "a refused call wrote to its outputs"

    def host(self):
        return (self.label.cpu().numpy(), self.dist.cpu().numpy(), self.counts.cpu().numpy(),
                self.inertia.cpu().numpy(), self.changed.cpu().numpy())


def _assign(X_d, N, D, C_d, K, label0):
    L = _lib()
    out = _Out(N, D, K, 0, label0)
    ins = G.Inputs(X=X_d, C=C_d)
    L.check(L.lib().cilrs_kmeans_assign(
        L.ptr(X_d), X_d.stride(0), N, D, L.ptr(C_d), C_d.stride(0), K, L.ptr(out.label), L.ptr(out.dist),
        L.ptr(out.counts), L.ptr(out.inertia), L.ptr(out.changed), L.ptr(out.scratch), out.nbytes, _st()))
    out.check()
    ins.check()
    return out.host()


def _update(X_d, N, D, label, C_d, K):
    """in place on C_d; returns counts"""
    L = _lib()
    out = _Out(N, D, K, 0, label)
    ins = G.Inputs(X=X_d, label=out.label)
    L.check(L.lib().cilrs_kmeans_update(
        L.ptr(X_d), X_d.stride(0), N, D, L.ptr(out.label), L.ptr(C_d), C_d.stride(0), K, L.ptr(out.counts),
        L.ptr(out.scratch), out.nbytes, _st()))
    out.check()
    ins.check()
    return out.counts.cpu().numpy()


def _lloyd(X_d, N, D, C_d, K, iters, label0=None):
    """in place on C_d; returns (label, dist, counts, inertia, changed) on the host"""
    L = _lib()
    out = _Out(N, D, K, iters, np.full(N, -1) if label0 is None else label0)
    ins = G.Inputs(X=X_d)
    L.check(L.lib().cilrs_kmeans_lloyd(
        L.ptr(X_d), X_d.stride(0), N, D, L.ptr(C_d), C_d.stride(0), K, iters, L.ptr(out.label),
        L.ptr(out.dist), L.ptr(out.counts), L.ptr(out.inertia), L.ptr(out.changed), L.ptr(out.scratch),
        out.nbytes, _st()))
    out.check()
    ins.check()
    return out.host()


def _pads_untouched(C_d, D):
    assert bool(torch.isnan(C_d[:, D:]).all()), "the pad columns of C were written"


# ---- assign ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 12, 260, 512, 1024, 2048])
@pytest.mark.parametrize("N", [1, 2, 5, 9, 257, 1030])
def test_assign_against_the_checker(N, D):
    X = KC.relu_rows(N, D, 11 * N + D)
    rng = np.random.default_rng(N + D)
    worst = 0.0
    for n, K in enumerate(k for k in KS[D] if k <= N):
        pad, padc = (0, 4) if n % 2 else (4, 0)
        Cn = KC.relu_rows(K, D, 500 + K + D)
        if K >= 3:
            Cn[1] = X[N // 2]                                # a centre that coincides with a row
        before = rng.integers(-1, K, size=N).astype(np.int32)
        label, dist, cnt, inertia, changed = _assign(_dev_rows(X, pad), N, D, _dev_rows(Cn, padc), K, before)
        worst = max(worst, KM.check_assign(X, Cn, before, label, dist, cnt, inertia[0], changed[0],
                                           f"N={N} D={D} K={K}"))
        if K >= 3:
            assert dist[N // 2] == 0.0 and label[N // 2] in (1, int(np.flatnonzero((Cn == Cn[1]).all(1))[0]))
    print(f"assign N={N} D={D}: largest share of the bound {worst:.3g}")


GRID_CASES = {
    # more rows than one pass of 256 workgroups x 16 (8) waves x ROWS[D] rows
    "n16389_d4": (16389, 4, 9),
    "n16389_d512_ld": (16389, 512, 3),
    "n4101_d1024": (4101, 1024, 3),
    "n2053_d2048": (2053, 2048, 3),
}


@pytest.mark.parametrize("case", list(GRID_CASES))
def test_assign_more_rows_than_one_grid_pass(case):
    N, D, K = GRID_CASES[case]
    X = KC.relu_rows(N, D, 3 + D)
    Cn = KC.relu_rows(K, D, 4 + D)
    before = np.full(N, -1, dtype=np.int32)
    label, dist, cnt, inertia, changed = _assign(_dev_rows(X, 4 if "ld" in case else 0), N, D,
                                                 _dev_rows(Cn, 0), K, before)
    share = KM.check_assign(X, Cn, before, label, dist, cnt, inertia[0], changed[0], case)
    print(f"assign {case}: share of the bound {share:.3g}")


@pytest.mark.parametrize("N,D,K", [(257, 12, 129), (257, 512, 65), (130, 2048, 17), (70, 1024, 33)])
def test_assign_equals_knn_over_the_centres_bit_for_bit(N, D, K):
    import test_knn_gpu as TKN
    X = KC.relu_rows(N, D, 21 + D)
    Cn = KC.relu_rows(K, D, 22 + D)
    Cn[K - 1] = Cn[2]                                        # duplicates: the lowest index wins
    Cn[5] = Cn[2]
    Cn[3, D // 2] = np.nan                                   # a NaN centre is no candidate
    X[7] = Cn[2]                                             # a row on the duplicated centre
    X[11, 1] = np.nan                                        # an all-NaN row: -1 / +inf
    X[12] = 3e19                                             # squares overflow: +inf is an ordinary value
    X_d, C_d = _dev_rows(X, 4), _dev_rows(Cn, 0)
    label, dist, cnt, _inertia, _changed = _assign(X_d, N, D, C_d, K, np.full(N, -1, dtype=np.int32))
    idx, kd = TKN._knn(C_d, K, D, X_d, N, 1)
    assert np.array_equal(label.astype(np.int64), idx[:, 0]), np.flatnonzero(label != idx[:, 0])
    assert np.array_equal(dist.view(np.uint32), kd[:, 0].view(np.uint32))
    assert label[7] == 2 and dist[7] == 0.0 and label[11] == -1 and dist[11] == np.inf
    assert label[12] == 0 and dist[12] == np.inf and 3 not in label.tolist()
    assert cnt.sum() == N - 1


# ---- update ------------------------------------------------------------------------------------------
def _int_rows(N, D, seed):
    return np.random.default_rng(seed).integers(0, 8, size=(N, D)).astype(np.float32)


@pytest.mark.parametrize("N,D,K", [(1, 4, 1), (9, 12, 3), (1030, 260, 7), (1030, 512, 65), (257, 2048, 5)])
def test_update_integer_rows_bit_for_bit(N, D, K):
    X = _int_rows(N, D, 5 + D)
    rng = np.random.default_rng(N + K)
    Cn = KC.relu_rows(K, D, 9)
    cases = {"random": rng.integers(0, K, size=N), "one cluster": np.full(N, K - 1),
             "some rows out": np.where(rng.random(N) < 0.3, -1, rng.integers(0, K, size=N))}
    if K > 2:
        hole = rng.integers(0, K - 1, size=N)
        cases["an empty cluster"] = np.where(hole >= 1, hole + 1, hole)      # nobody takes label 1
    for name, label in cases.items():
        label = label.astype(np.int32)
        for pad in (0, 4):
            C_d = _dev_rows(Cn, pad)
            cnt = _update(_dev_rows(X, 4 - pad), N, D, label, C_d, K)
            assert np.array_equal(cnt, KM.counts(label, K)), (name, cnt)
            _pads_untouched(C_d, D)
            KM.check_update(X, label, Cn, C_d[:, :D].cpu().numpy(), exact=True, what=f"{name} pad={pad}")


def test_update_relu_rows_within_one_ulp():
    N, D, K = 1030, 512, 9
    X = KC.relu_rows(N, D, 77)
    label = np.random.default_rng(1).integers(-1, K, size=N).astype(np.int32)
    Cn = KC.relu_rows(K, D, 78)
    C_d = _dev_rows(Cn, 0)
    _update(_dev_rows(X, 0), N, D, label, C_d, K)
    off = KM.check_update(X, label, Cn, C_d.cpu().numpy())
    print(f"update: {off:.3g} of the centre entries one ulp from the rounded float64 mean")


# ---- lloyd -------------------------------------------------------------------------------------------
def _walk(X_d, N, D, C0, K, iters):
    """`iters` iterations one call at a time: the device's own sequence for the checker"""
    C_d = _dev_rows(C0, 0)
    label = np.full(N, -1, dtype=np.int32)
    steps = []
    for t in range(iters + 1):
        Ct = C_d.cpu().numpy()
        new, dist, cnt, inertia, changed = _lloyd(X_d, N, D, C_d, K, 0, label)
        steps.append((Ct, new, dist, cnt, inertia[0], changed[0]))
        if t < iters:
            _update(X_d, N, D, new, C_d, K)
        label = new
    return steps, C_d


def test_lloyd_random_rows_through_the_walking_checker():
    N, D, K, iters = 1030, 512, 9, 10
    X = KC.relu_rows(N, D, 91)
    X_d = _dev_rows(X, 4)
    C0 = X[:K].copy()
    steps, C_walk = _walk(X_d, N, D, C0, K, iters)
    J = KM.check_steps(X, C0, np.full(N, -1, dtype=np.int32), steps, "relu rows")
    print("lloyd: J64 " + " ".join(f"{j:.6g}" for j in J))
    # one call is the walk, bit for bit; so are two calls, and a second run
    C_one = _dev_rows(C0, 0)
    label, dist, cnt, inertia, changed = _lloyd(X_d, N, D, C_one, K, iters)
    assert torch.equal(C_one, C_walk)
    assert np.array_equal(label, steps[-1][1]) and np.array_equal(dist.view(np.uint32), steps[-1][2].view(np.uint32))
    assert np.array_equal(cnt, steps[-1][3])
    assert np.array_equal(inertia, np.array([s[4] for s in steps]))
    assert np.array_equal(changed, np.array([s[5] for s in steps]))
    C_two = _dev_rows(C0, 4)
    l1, _d1, _c1, i1, ch1 = _lloyd(X_d, N, D, C_two, K, 4)
    l2, d2, c2, i2, ch2 = _lloyd(X_d, N, D, C_two, K, iters - 4, l1)
    _pads_untouched(C_two, D)
    assert torch.equal(C_two[:, :D], C_one) and np.array_equal(l2, label) and np.array_equal(c2, cnt)
    assert np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
    assert ch2[0] == 0 and i2[0] == i1[-1]                   # the second call's first assign repeats
    assert np.array_equal(np.concatenate([i1, i2[1:]]), inertia)
    assert np.array_equal(np.concatenate([ch1, ch2[1:]]), changed)
    C_again = _dev_rows(C0, 0)
    again = _lloyd(X_d, N, D, C_again, K, iters)
    assert torch.equal(C_again, C_one)
    for a, b in zip(again, (label, dist, cnt, inertia, changed)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_lloyd_with_no_iteration_is_the_closing_assign():
    N, D, K = 257, 260, 9
    X, Cn = KC.relu_rows(N, D, 1), KC.relu_rows(K, D, 2)
    X_d, C_d = _dev_rows(X, 0), _dev_rows(Cn, 4)
    before = np.zeros(N, dtype=np.int32)
    got = _lloyd(X_d, N, D, C_d, K, 0, before)
    assert torch.equal(C_d[:, :D].cpu(), torch.from_numpy(Cn))
    _pads_untouched(C_d, D)
    want = _assign(X_d, N, D, C_d, K, before)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_lloyd_recovers_planted_blobs_and_stays_at_the_fixed_point():
    K, per, D = 9, 30, 260
    X, truth = KM.blobs(K, per, D, 5)
    N = len(X)
    X_d = _dev_rows(X, 0)
    sel, _radius, _m = KC.greedy(X, np.full(N, np.inf), K)   # one row per blob (test_kmeans_host.py)
    C_d = _dev_rows(X[sel], 0)
    label, dist, cnt, inertia, changed = _lloyd(X_d, N, D, C_d, K, 6)
    assert KM.same_partition(label, truth) and (cnt == per).all()
    first = int(np.flatnonzero(changed == 0)[0])
    assert first <= 2 and (changed[first:] == 0).all()
    assert (inertia[first:] == inertia[first]).all()
    at_rest = C_d.clone()
    more = _lloyd(X_d, N, D, C_d, K, 3, label)               # past convergence: bit-identical
    assert torch.equal(C_d, at_rest) and not more[4].any()
    assert np.array_equal(more[0], label) and np.array_equal(more[1].view(np.uint32), dist.view(np.uint32))
    KM.check_update(X, label, X[sel], C_d.cpu().numpy(), what="blobs")


# ---- the scratch query and the refusals ------------------------------------------------------------
def test_scratch_size_query():
    lib = _lib().lib()
    for N, D, K in ((1, 4, 1), (1030, 512, 9), (176256, 512, 64), (176256, 512, 256), (1 << 24, 2048, 1024)):
        n = lib.cilrs_kmeans_scratch_bytes(N, D, K)
        assert n > 0 and n % 16 == 0 and n >= 4 * N
    assert lib.cilrs_kmeans_scratch_bytes(176256, 512, 64) < 8 << 20
    for N, D, K in ((0, 4, 1), ((1 << 24) + 1, 4, 1), (5, 0, 1), (5, 6, 1), (5, 2052, 1), (5, 4, 0), (5, 4, 6),
                    (2000, 4, 1025)):
        assert lib.cilrs_kmeans_scratch_bytes(N, D, K) == 0


def _refusal_args():
    N, D, K = 5, 12, 3
    X_d = _dev_rows(KC.relu_rows(N, D, 1), 4)
    C_d = _dev_rows(KC.relu_rows(K, D, 2), 4)
    return dict(X=X_d, ld=X_d.stride(0), N=N, D=D, C=C_d, ldc=C_d.stride(0), K=K, iters=2)


def _off(t, nbytes):
    return None if t is None else C.c_void_p(t.data_ptr() + nbytes)


REFUSALS = {
    "null X": (dict(X=None), "NULL"),
    "null C": (dict(C=None), "NULL"),
    "null label": (dict(null="label"), "NULL"),
    "null dist": (dict(null="dist"), "NULL"),
    "null counts": (dict(null="counts"), "NULL"),
    "null inertia": (dict(null="inertia"), "NULL"),
    "null changed": (dict(null="changed"), "NULL"),
    "N 0": (dict(N=0), "N ="),
    "N above 2^24": (dict(N=(1 << 24) + 1), "N ="),
    "D 0": (dict(D=0), "D ="),
    "D 6": (dict(D=6, ld=8, ldc=8), "D ="),
    "D 2052": (dict(D=2052, ld=2052, ldc=2052), "D ="),
    "ld below D": (dict(ld=8), "ld ="),
    "ld 14": (dict(ld=14), "ld ="),
    "ldc below D": (dict(ldc=8), "ldc ="),
    "ldc 18": (dict(ldc=18), "ldc ="),
    "X off by 4 bytes": (dict(X_off=4), "aligned"),
    "C off by 8 bytes": (dict(C_off=8), "aligned"),
    "K 0": (dict(K=0), "K ="),
    "K above N": (dict(K=6), "K ="),
    "K above 1024": (dict(K=1025, N=2000), "K ="),
    "iters negative": (dict(iters=-1), "iters ="),
    "iters 10001": (dict(iters=10001), "iters ="),
    "null scratch": (dict(null="scratch"), "scratch"),
    "scratch one byte short": (dict(short=1), "scratch"),
    "scratch off by 8 bytes": (dict(scratch_off=8), "aligned"),
}


def _applies(entry, change):
    """is the changed argument one of this entry's?"""
    if "iters" in change:
        return entry == "lloyd"
    return entry != "update" or change.get("null") not in ("dist", "inertia", "changed")


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("assign", "update", "lloyd") for c in REFUSALS
                                        if _applies(e, REFUSALS[c][0])])
def test_refusals_launch_nothing(entry, case):
    change, text = REFUSALS[case]
    a = _refusal_args()
    a.update(change)
    L = _lib()
    null, off = a.get("null"), a.get("scratch_off", 0)
    out = _Out(5, 12, 3, 2, short=a.get("short", 0), extra=16 if off else 0)
    before = None if a["C"] is None else a["C"].clone()
    p = lambda name: None if null == name else L.ptr(getattr(out, name))
    X, Cc = _off(a["X"], a.get("X_off", 0)), _off(a["C"], a.get("C_off", 0))
    scratch = None if null == "scratch" else _off(out.scratch, off)
    nbytes = out.nbytes - a.get("short", 0)
    if entry == "assign":
        rc = L.lib().cilrs_kmeans_assign(X, a["ld"], a["N"], a["D"], Cc, a["ldc"], a["K"], p("label"), p("dist"),
                                         p("counts"), p("inertia"), p("changed"), scratch, nbytes, _st())
    elif entry == "update":
        rc = L.lib().cilrs_kmeans_update(X, a["ld"], a["N"], a["D"], p("label"), Cc, a["ldc"], a["K"], p("counts"),
                                         scratch, nbytes, _st())
    else:
        rc = L.lib().cilrs_kmeans_lloyd(X, a["ld"], a["N"], a["D"], Cc, a["ldc"], a["K"], a["iters"], p("label"),
                                        p("dist"), p("counts"), p("inertia"), p("changed"), scratch, nbytes, _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    out.untouched()
    if before is not None:
        assert torch.equal(a["C"].view(torch.int32), before.view(torch.int32)), "a refused call wrote to C"


# ---- end to end --------------------------------------------------------------------------------------
def test_end_to_end_frame_pool_cluster(tmp_path):
    import cilrs_oracle as O
    import test_novelty_gpu as TN
    from cilrs_mi355 import Clustering, FramePool
    m, _orc = TM._pair()
    fd, _feats = TN._fitted_density()
    pool = FramePool(m, 24)
    for i, B in enumerate((3, 5, 3, 5, 5, 3)):
        img, spd, cmd, _t, _u8 = O.synthetic_batch(B, seed=900 + i, h=40, w=120)
        pool.add(img.cuda(), spd.cuda(), cmd.cuda())
    for density in (None, fd):
        c = pool.cluster(4, density=density, iters=20, check_every=3)
        assert isinstance(c, Clustering) and c.metric == ("euclidean" if density is None else "mahalanobis")
        assert tuple(c.centres.shape) == (4, 512) and c.centres.is_cuda and c.labels.dtype == torch.int32
        assert tuple(c.labels.shape) == tuple(c.dist.shape) == (24,) and c.sizes.dtype == np.int64
        assert c.converged and c.changed[c.iterations] == 0 and len(c.inertia) == len(c.changed)
        assert c.sizes.sum() == 24 and np.array_equal(c.sizes, KM.counts(c.labels.cpu().numpy(), 4))
        # the closing assignment against the checker, on the rows the clustering ran on
        Z = c.rows.cpu().numpy()
        last = len(c.changed) - 1
        KM.check_assign(Z, c.centres.cpu().numpy(), c.labels.cpu().numpy(), c.labels.cpu().numpy(),
                        c.dist.cpu().numpy(), c.sizes, c.inertia[last], 0, "end to end")
        KM.check_update(Z, c.labels.cpu().numpy(), c.centres.cpu().numpy(), c.centres.cpu().numpy(),
                        what="end to end: the centres are the means of their rows")
        labels, dist = c.assign(pool.features())             # through the whitening and cilrs_knn
        assert torch.equal(labels, c.labels) and torch.equal(dist.view(torch.int32), c.dist.view(torch.int32))
        med = c.medoids()
        assert med.dtype == np.int64 and np.array_equal(c.labels.cpu().numpy()[med], np.arange(4))
        assert np.array_equal(c.histogram(pool.features()), c.sizes)
        w = c.balanced_weights()
        for k in range(4):
            assert abs(w[c.labels.cpu().numpy() == k].sum() - 24 / 4) < 1e-12
        c.save(tmp_path / "c.pt")
        back = Clustering.load(tmp_path / "c.pt", device="cuda")
        assert torch.equal(back.centres, c.centres) and torch.equal(back.labels, c.labels)
        assert np.array_equal(back.histogram(pool.features()), c.sizes)
    # seeds given as rows and as centres agree; a change of check_every changes nothing
    rows = torch.tensor([0, 5, 9], dtype=torch.int64)
    a = pool.cluster(3, init=rows, iters=8, check_every=1)
    b = pool.cluster(3, init=pool.features()[rows.cuda()].clone(), iters=8, check_every=8)
    assert torch.equal(a.centres, b.centres) and torch.equal(a.labels, b.labels)
    assert np.array_equal(a.inertia[:a.iterations + 1], b.inertia[:a.iterations + 1])
