"""Greedy k-center on the device (csrc/kcenter.hip: cilrs_kcenter_cover, cilrs_kcenter_greedy,
cilrs_mi355.select.FramePool) against the float64 definition of tests/_kcenter.py.

Gates.  A distance: (4 ceil(D / 256) + 9) 2^-24 relative (tests/_kcenter.py, bound).  The greedy
tests walk the device's own sequence of picks (check_greedy), so a near-tie between two rows cannot
make them flaky; rows with small integer entries make every fp32 sum exact, and there sel, radius
and mind must equal the definition bit for bit, ties included.

What the cases cross.  The cover kernel holds CHUNK = 8 centres in LDS per pass over the rows: M = 1,
3 stay inside one chunk, 9 and 17 cross it.  Both kernels run at most 1,024 workgroups of 4 waves
and a wave takes ROWS[D] rows at a time (4 up to D = 512, 2 up to 1,024, else 1): one pass of the
grid covers 4,096 * ROWS[D] rows, and N = that + 5 makes some waves loop.  Outputs are NaN- (sel:
-1-) pre-filled inside guard bands (tests/_guards.py), the scratch is exactly
cilrs_kcenter_scratch_bytes, the pad columns of X and C hold NaN: they must not be read.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _guards as G
import _kcenter as K
import cilrs_oracle as O
import test_mc_dropout_gpu as TM

pytestmark = pytest.mark.gpu

CHUNK = 8
GRID_WAVES = 1024 * 4


def rows_per_wave(D):
    return 4 if D <= 512 else 2 if D <= 1024 else 1


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    msg = _lib().lib().cilrs_last_error()
    return msg.decode() if msg else ""


def _dev_rows(X, pad):
    """[N][D + pad] on the device, the pad columns NaN"""
    return TM._pooled_dev(torch.from_numpy(X), X.shape[1] + pad)


def _guarded_mind(mind0):
    m, check = G.guarded(len(mind0), name="mind")
    m.copy_(torch.from_numpy(np.asarray(mind0, dtype=np.float32)))
    return m, check


def _cover(X_d, N, D, C_d, M, mind):
    L = _lib()
    L.check(L.lib().cilrs_kcenter_cover(L.ptr(X_d), X_d.stride(0), N, D, L.ptr(C_d),
                                        0 if C_d is None else C_d.stride(0), M, L.ptr(mind), _st()))


class _Picks:
    """guarded sel / radius and an exactly sized scratch"""

    def __init__(self, N, Kp, short=0, extra=0):
        self.nbytes = _lib().lib().cilrs_kcenter_scratch_bytes(N)
        self.sel, c1 = G.guarded(Kp, dtype=torch.int64, fill=-1, name="sel")
        self.radius, c2 = G.guarded(Kp, name="radius")
        self.scratch, c3 = G.guarded(max(self.nbytes - short + extra, 1), dtype=torch.uint8, fill=0xA5,
                                     name="scratch")
        self.checks = (c1, c2, c3)

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        assert bool((self.sel == -1).all()) and bool(torch.isnan(self.radius).all()) and \
            bool((self.scratch == 0xA5).all()), "a refused call wrote to its outputs"


def _greedy(X_d, N, D, mind, Kp):
    """Kp picks on a guarded mind; returns (sel, radius) on the host after every band was checked"""
    L = _lib()
    out = _Picks(N, Kp)
    ins = G.Inputs(X=X_d)
    L.check(L.lib().cilrs_kcenter_greedy(L.ptr(X_d), X_d.stride(0), N, D, L.ptr(mind), Kp,
                                         L.ptr(out.sel), L.ptr(out.radius), L.ptr(out.scratch),
                                         out.nbytes, _st()))
    out.check()
    ins.check()
    return out.sel.cpu().numpy(), out.radius.cpu().numpy()


# ---- cover -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 12, 260, 512, 2048])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_cover_against_float64(N, D):
    X = K.relu_rows(N, D, 7 * N + D)
    worst = 0.0
    for pad in (0, 4):
        X_d = _dev_rows(X, pad)
        for M in (1, 3, 9, 17):
            Cn = K.relu_rows(M, D, 1000 + M + D)
            if M >= 3 and N > 1:
                Cn[1] = X[N // 2]                            # a centre that coincides with a row
            C_d = _dev_rows(Cn, 4 - pad)
            dmin = K.cover(X, Cn, np.full(N, np.inf))
            # a finite start: every other entry below every distance, the rest above the nearest
            finite = (dmin * np.where(np.arange(N) % 2 == 0, 0.5, 2.0) + 1e-3).astype(np.float32)
            for start in (np.full(N, np.inf, dtype=np.float32), finite):
                mind, check = _guarded_mind(start)
                ins = G.Inputs(X=X_d, C=C_d)
                _cover(X_d, N, D, C_d, M, mind)
                check()
                ins.check()
                got = mind.cpu().numpy()
                worst = max(worst, K.check_cover(X, Cn, start, got, f"N={N} D={D} pad={pad} M={M}"))
                if M >= 3 and N > 1 and np.isinf(start[0]):
                    assert got[N // 2] == 0.0
                below = start.astype(np.float64) < (1.0 - K.bound(D)) * dmin
                assert np.isinf(start[0]) or (below.any() and (N == 1 or not below.all())), \
                    "the finite start must have entries on both sides"
                # centre by centre is bit for bit all centres at once (the chunks keep the order)
                one, check1 = _guarded_mind(start)
                for m in range(M):
                    _cover(X_d, N, D, C_d[m:m + 1], 1, one)
                check1()
                assert torch.equal(one, mind), (N, D, pad, M)
    print(f"cover N={N} D={D}: largest share of the bound {worst:.3g}")


# ---- greedy ----------------------------------------------------------------------------------------
GREEDY_SHAPES = {
    # name: (N, D, pad, picks)
    "n1_d4": (1, 4, 0, (1,)),
    "n3_d12_ld": (3, 12, 4, (1, 2, 3)),
    "n5_d260": (5, 260, 0, (1, 2, 5)),
    "n5_d2048_ld": (5, 2048, 4, (1, 2, 5)),
    "n257_d4_ld": (257, 4, 4, (1, 2, 37, 257)),
    "n257_d512": (257, 512, 0, (1, 2, 37, 257)),
    "n257_d1024_ld": (257, 1024, 4, (1, 2, 37, 257)),
    "n257_d2048": (257, 2048, 0, (1, 2, 37, 257)),
    # one pass of the grid covers GRID_WAVES * rows_per_wave(D) rows: these make some waves loop
    "n16389_d4": (GRID_WAVES * 4 + 5, 4, 0, (1, 2, 37, GRID_WAVES * 4 + 5)),
    "n16389_d512_ld": (GRID_WAVES * 4 + 5, 512, 4, (3,)),
    "n8197_d1024": (GRID_WAVES * 2 + 5, 1024, 0, (3,)),
    "n4101_d2048": (GRID_WAVES + 5, 2048, 0, (3,)),
}


@pytest.mark.parametrize("case", list(GREEDY_SHAPES))
def test_greedy_random_rows_through_the_checker(case):
    N, D, pad, picks = GREEDY_SHAPES[case]
    assert N <= GRID_WAVES * rows_per_wave(D) or N == GRID_WAVES * rows_per_wave(D) + 5
    X = K.relu_rows(N, D, 31 + N + D)
    X_d = _dev_rows(X, pad)
    Cn = K.relu_rows(3, D, 5)
    covered = K.cover(X, Cn, np.full(N, np.inf)).astype(np.float32)
    for Kp in picks:
        for name, start in (("inf", np.full(N, np.inf, dtype=np.float32)), ("covered", covered)):
            if name == "covered" and Kp > 37:
                continue                                     # the long runs once
            mind, check = _guarded_mind(start)
            sel, radius = _greedy(X_d, N, D, mind, Kp)
            check()
            share, ratio = K.check_greedy(X, start, sel, radius, mind.cpu().numpy(),
                                          f"{case} K={Kp} {name}")
            if name == "inf":
                assert sel[0] == 0 and radius[0] == np.inf
            live = sel[radius > 0]                           # relu rows at D = 4 repeat (all zeros)
            assert len(set(live.tolist())) == len(live), "no row is picked twice at a radius > 0"
    print(f"greedy {case}: share of the bound {share:.3g}, worst pick at {ratio:.9f} of the farthest")


def _int_rows(N, D, seed, distinct=None):
    rng = np.random.default_rng(seed)
    if distinct is None:
        return rng.integers(0, 8, size=(N, D)).astype(np.float32)
    base = rng.integers(0, 8, size=(distinct, D)).astype(np.float32)
    assert len({r.tobytes() for r in base}) == distinct
    return base[np.arange(N) % distinct]


EXACT_CASES = {
    # name: (N, D, pad, distinct rows, picks); every fp32 sum is an exact integer <= 2048 * 49 < 2^24
    "n12_d4_4distinct": (12, 4, 0, 4, 6),
    "n12_d260_4distinct_ld": (12, 260, 4, 4, 6),
    "n12_d2048_4distinct": (12, 2048, 0, 4, 6),
    "n257_d4": (257, 4, 4, None, 37),
    "n257_d512": (257, 512, 0, None, 37),
    "n16389_d4_ties_across_workgroups": (GRID_WAVES * 4 + 5, 4, 0, None, 37),
}


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_greedy_integer_rows_equal_the_definition_bit_for_bit(case):
    N, D, pad, distinct, Kp = EXACT_CASES[case]
    X = _int_rows(N, D, 3 + D, distinct)
    X_d = _dev_rows(X, pad)
    for start in (np.full(N, np.inf, dtype=np.float32),
                  K.cover(X, _int_rows(2, D, 9), np.full(N, np.inf)).astype(np.float32)):
        want_sel, want_radius, want_mind = K.greedy(X, start, Kp)
        mind, check = _guarded_mind(start)
        sel, radius = _greedy(X_d, N, D, mind, Kp)
        check()
        assert torch.equal(torch.from_numpy(sel), torch.from_numpy(want_sel)), (case, sel, want_sel)
        assert torch.equal(torch.from_numpy(radius), torch.from_numpy(want_radius.astype(np.float32)))
        assert torch.equal(mind.cpu(), torch.from_numpy(want_mind.astype(np.float32)))
        if distinct is not None and np.isinf(start[0]):
            assert (radius[distinct:] == 0).all() and (sel[distinct:] == 0).all()
            assert (radius[:distinct] > 0).all() and not mind.any()


def test_greedy_invariants():
    N, D = 257, 512
    X = K.relu_rows(N, D, 77)
    X_d = _dev_rows(X, 4)
    start = np.full(N, np.inf, dtype=np.float32)
    m8, c8 = _guarded_mind(start)
    sel8, rad8 = _greedy(X_d, N, D, m8, 8)
    assert sel8[0] == 0 and rad8[0] == np.inf                # the +inf start picks row 0
    m53, c53 = _guarded_mind(start)
    sel5, rad5 = _greedy(X_d, N, D, m53, 5)
    sel3, rad3 = _greedy(X_d, N, D, m53, 3)
    c8()
    c53()
    assert np.array_equal(np.concatenate([sel5, sel3]), sel8)
    assert np.array_equal(np.concatenate([rad5, rad3]).view(np.uint32), rad8.view(np.uint32))
    assert torch.equal(m53, m8)
    again, _c = _guarded_mind(start)                         # two runs are bit-identical
    sel_b, rad_b = _greedy(X_d, N, D, again, 8)
    assert np.array_equal(sel_b, sel8) and np.array_equal(rad_b.view(np.uint32), rad8.view(np.uint32))
    assert torch.equal(again, m8)
    # NaN entries never win; a NaN in mind[0] is never beaten
    nan_mid = start.copy()
    nan_mid[3] = np.nan
    m, _c = _guarded_mind(nan_mid)
    sel, _r = _greedy(X_d, N, D, m, 4)
    assert 3 not in sel.tolist() and sel[0] == 0 and bool(torch.isnan(m[3]))
    nan0 = K.cover(X, K.relu_rows(1, D, 2), start).astype(np.float32)
    nan0[0] = np.nan
    m, _c = _guarded_mind(nan0)
    sel, rad = _greedy(X_d, N, D, m, 2)
    assert sel.tolist() == [0, 0] and np.isnan(rad).all()


def test_scratch_size_query():
    lib = _lib().lib()
    for N in (1, 3, 4096, 4097, 176256, 1 << 24):
        n = lib.cilrs_kcenter_scratch_bytes(N)
        assert 0 < n <= 2 * 1024 * 8 and n % 16 == 0
    for N in (0, -1, (1 << 24) + 1):
        assert lib.cilrs_kcenter_scratch_bytes(N) == 0


# ---- refusals ----------------------------------------------------------------------------------------
def _refusal_args():
    N, D = 5, 12
    X_d = _dev_rows(K.relu_rows(N, D, 1), 4)
    C_d = _dev_rows(K.relu_rows(3, D, 2), 4)
    return dict(X=X_d, ld=X_d.stride(0), N=N, D=D, C=C_d, ldc=C_d.stride(0), M=3, K=2)


def _off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


COMMON_REFUSALS = {
    "null X": (dict(X=None), "NULL"),
    "null mind": (dict(null="mind"), "NULL"),
    "N 0": (dict(N=0), "N ="),
    "N above 2^24": (dict(N=(1 << 24) + 1), "N ="),
    "D 0": (dict(D=0), "D ="),
    "D 6": (dict(D=6, ld=8), "D ="),
    "D 2052": (dict(D=2052, ld=2052), "D ="),
    "ld below D": (dict(ld=8), "ld ="),
    "ld 14": (dict(ld=14), "ld ="),
    "X off by 4 bytes": (dict(X_off=4), "aligned"),
}
COVER_REFUSALS = dict(COMMON_REFUSALS, **{
    "null C": (dict(C=None), "NULL"),
    "M negative": (dict(M=-1), "M ="),
    "M 65537": (dict(M=65537), "M ="),
    "ldc below D": (dict(ldc=8), "ldc ="),
    "ldc 18": (dict(ldc=18), "ldc ="),
    "C off by 8 bytes": (dict(C_off=8), "aligned"),
})
GREEDY_REFUSALS = dict(COMMON_REFUSALS, **{
    "null sel": (dict(null="sel"), "NULL"),
    "null radius": (dict(null="radius"), "NULL"),
    "K 0": (dict(K=0), "K ="),
    "K above N": (dict(K=6), "K ="),
    "null scratch": (dict(null="scratch"), "scratch"),
    "scratch one byte short": (dict(short=1), "scratch"),
    "scratch off by 8 bytes": (dict(scratch_off=8), "aligned"),
})


def _xptr(a):
    return None if a["X"] is None else _off(a["X"], a.get("X_off", 0))


@pytest.mark.parametrize("case", list(COVER_REFUSALS))
def test_cover_refusals_launch_nothing(case):
    change, text = COVER_REFUSALS[case]
    a = _refusal_args()
    a.update(change)
    L = _lib()
    mind, check = G.guarded(5, name="mind")
    rc = L.lib().cilrs_kcenter_cover(
        _xptr(a), a["ld"], a["N"], a["D"], None if a["C"] is None else _off(a["C"], a.get("C_off", 0)),
        a["ldc"], a["M"], None if a.get("null") == "mind" else L.ptr(mind), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    check()
    assert bool(torch.isnan(mind).all())


@pytest.mark.parametrize("case", list(GREEDY_REFUSALS))
def test_greedy_refusals_launch_nothing(case):
    change, text = GREEDY_REFUSALS[case]
    a = _refusal_args()
    a.update(change)
    L = _lib()
    null, off = a.get("null"), a.get("scratch_off", 0)
    out = _Picks(5, 2, short=a.get("short", 0), extra=16 if off else 0)
    mind, check = G.guarded(5, name="mind")
    rc = L.lib().cilrs_kcenter_greedy(
        _xptr(a), a["ld"], a["N"], a["D"], None if null == "mind" else L.ptr(mind), a["K"],
        None if null == "sel" else L.ptr(out.sel), None if null == "radius" else L.ptr(out.radius),
        None if null == "scratch" else _off(out.scratch, off), out.nbytes - a.get("short", 0), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    check()
    out.untouched()
    assert bool(torch.isnan(mind).all())


def test_cover_with_no_centre_is_a_successful_no_op():
    a = _refusal_args()
    L = _lib()
    mind, check = G.guarded(5, name="mind")
    assert L.lib().cilrs_kcenter_cover(L.ptr(a["X"]), a["ld"], 5, 12, None, 0, 0, L.ptr(mind), _st()) == 0
    check()
    assert bool(torch.isnan(mind).all())


# ---- end to end --------------------------------------------------------------------------------------
def test_end_to_end_frame_pool():
    import test_novelty_gpu as TN
    from cilrs_mi355 import FramePool
    m, _orc = TM._pair()
    fd, _feats = TN._fitted_density()                        # fitted on 40 other frames
    eng = m.engine()
    F = 512
    with pytest.raises(RuntimeError, match="fp32 only"):
        FramePool(m, 24, half=True)
    pool = FramePool(m, 24)
    left = []
    for i, B in enumerate((3, 5, 3, 5, 5, 3)):
        img, spd, cmd, _t, _u8 = O.synthetic_batch(B, seed=900 + i, h=40, w=120)
        assert pool.add(img.cuda(), spd.cuda(), cmd.cuda()) is pool
        left.append(eng.plan_features(eng.last_plan).clone())
    assert len(pool) == 24 and tuple(pool.features().shape) == (24, F)
    assert torch.equal(pool.features(), torch.cat(left))
    with pytest.raises(RuntimeError, match="full"):
        pool.add(img.cuda(), spd.cuda(), cmd.cuda())
    # Mahalanobis metric: the checker on the pool's own whitened rows, from the float64 cover of the
    # fit's command means
    s = pool.select(8, density=fd)
    assert s.metric == "mahalanobis" and s.indices.dtype == np.int64 and s.radius.dtype == np.float32
    assert len(s.indices) == 8 and tuple(s.min_dist.shape) == (24,) and s.min_dist.is_cuda
    Z = s.rows.cpu().numpy()
    assert Z.shape == (24, F)
    # the library product against float64 of the same fp32 tables: F products and their sums
    k0 = int(np.flatnonzero(fd.present)[0])
    W64 = np.tril(fd.W.cpu().numpy().astype(np.float64))
    u = (pool.features().cpu().numpy() - fd.mean.cpu().numpy()[k0]).astype(np.float64)
    assert (np.abs(Z - u @ W64.T) <= (F + 2) * 2.0 ** -24 * (np.abs(u) @ np.abs(W64).T)).all()
    start = K.cover(Z, fd.whitened_means().cpu().numpy(), np.full(24, np.inf))
    share, ratio = K.check_greedy(Z, start, s.indices, s.radius, s.min_dist.cpu().numpy(), "whitened")
    print(f"end to end, whitened: share of the bound {share:.3g}, worst pick at {ratio:.9f}; "
          f"coverage {s.coverage()[0]:.4g} .. {s.coverage()[-1]:.4g}")
    assert np.isfinite(s.radius).all() and (np.diff(s.radius) <= 0).all()
    assert np.array_equal(s.coverage(), np.sqrt(s.radius))
    # Euclidean metric on the raw rows
    e = pool.select(8)
    assert e.metric == "euclidean" and e.indices[0] == 0 and e.radius[0] == np.inf
    raw = pool.features().cpu().numpy()
    K.check_greedy(raw, np.full(24, np.inf), e.indices, e.radius, e.min_dist.cpu().numpy(), "raw")
    f = pool.select(4, first=7)
    assert f.indices[0] == 7 and f.radius[0] == np.inf
    K.check_greedy(raw, K.dist(raw, raw[7]), f.indices[1:], f.radius[1:], f.min_dist.cpu().numpy(),
                   "raw, first = 7")
    # what was chosen before is covered: the second selection is disjoint from the first
    chosen = pool.features()[torch.from_numpy(s.indices).cuda()]
    s2 = pool.select(8, density=fd, covered=chosen)
    assert len(s2.indices) == 8 and not set(s2.indices.tolist()) & set(s.indices.tolist())
    start2 = K.cover(Z, fd.whiten(chosen).cpu().numpy(), start)   # the centres as the device took them
    K.check_greedy(Z, start2, s2.indices, s2.radius, s2.min_dist.cpu().numpy(), "whitened, covered")
    # a change of the weights between two adds raises
    room = FramePool(m, 8)
    img, spd, cmd, _t, _u8 = O.synthetic_batch(3, seed=950, h=40, w=120)
    room.add(img.cuda(), spd.cuda(), cmd.cuda())
    m.weights_changed()
    with pytest.raises(RuntimeError, match="weights changed"):
        room.add(img.cuda(), spd.cuda(), cmd.cuda())
    assert len(room) == 3
