"""Greedy k-center in float64: the definition of include/cilrs_hip.h ("Greedy k-center") restated
with numpy, and the checker the device tests go through (test_kcenter_host.py,
test_kcenter_gpu.py)."""
import numpy as np


def relu_rows(N, D, seed, scale=1.0):
    """post-ReLU shaped rows: relu of a Gaussian, fp32 [N][D]"""
    rng = np.random.default_rng(seed)
    return (np.maximum(rng.standard_normal((N, D)), 0.0) * scale).astype(np.float32)


def dist(X, c):
    """d(X_i, c) = sum_j (X_ij - c_j)^2 for every row, in float64 of the fp32 values"""
    t = np.asarray(X, dtype=np.float32).astype(np.float64) - \
        np.asarray(c, dtype=np.float32).astype(np.float64)[None, :]
    return np.einsum("ij,ij->i", t, t)


def lower(m, d):
    """min(a, b) = b < a ? b : a, elementwise: a NaN distance never replaces a value"""
    with np.errstate(invalid="ignore"):
        return np.where(d < m, d, m)


def cover(X, C, mind):
    """mind after the centres C [M][D], in order"""
    m = np.array(mind, dtype=np.float64)
    for c in np.asarray(C, dtype=np.float32).reshape(-1, np.asarray(X).shape[1]):
        m = lower(m, dist(X, c))
    return m


def argmax_low(m):
    """index of the largest entry, the lowest index among equal values, from (m[0], 0): NaN entries
    never win, a NaN in m[0] is never beaten"""
    if np.isnan(m[0]):
        return 0
    return int(np.argmax(np.where(np.isnan(m), -np.inf, m)))


def greedy(X, mind, K):
    """(sel int64 [K], radius float64 [K], mind float64 [N]) of the definition"""
    m = np.array(mind, dtype=np.float64)
    sel, radius = np.zeros(K, dtype=np.int64), np.zeros(K)
    for t in range(K):
        i = argmax_low(m)
        sel[t], radius[t] = i, m[i]
        m = lower(m, dist(X, X[i]))
    return sel, radius, m


def bound(D):
    """Relative error of one fp32 distance against float64: two roundings from squaring a rounded
    difference, one per fma of a lane's chain (4 ceil(D / 256) of them), six for the butterfly, one
    spare.  Every term is non-negative, so the bound is relative; a minimum of such distances and a
    value taken from them keep it."""
    return (4 * -(-D // 256) + 9) * 2.0 ** -24


def close(got, want, b):
    """|got - want| <= b * want elementwise, infinities equal"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    ok = np.where(inf, got == want, np.abs(np.where(inf, 0.0, got) - np.where(inf, 0.0, want))
                  <= b * np.where(inf, 0.0, want))
    return ok


def check_cover(X, C, mind0, mind, what="cover"):
    """the device's mind after a cover against the definition; returns the largest share of the
    bound used.  Entries the centres did not lower must come back bit for bit."""
    D = np.asarray(X).shape[1]
    b = bound(D)
    m0 = np.asarray(mind0, dtype=np.float32)
    dmin = cover(X, C, np.full(len(m0), np.inf))
    want = lower(m0.astype(np.float64), dmin)
    got = np.asarray(mind, dtype=np.float32)
    kept = m0.astype(np.float64) < (1.0 - b) * dmin          # below every fp32 distance as well
    assert np.array_equal(got[kept].view(np.uint32), m0[kept].view(np.uint32)), \
        f"{what}: an entry below every distance was changed"
    ok = close(got, want, b)
    assert ok.all(), (what, got[~ok], want[~ok])
    fin = np.isfinite(want) & (want > 0)
    return float((np.abs(got[fin] - want[fin]) / (b * want[fin])).max()) if fin.any() else 0.0


def check_greedy(X, mind0, sel, radius, mind, what="greedy"):
    """Walk the DEVICE'S OWN sequence (a near-tie cannot make a test flaky): m64 is the float64
    running minimum under the centres the device chose.  Requires at every step
    m64[sel[t]] >= (1 - 2 bound) max(m64) and radius[t] within bound * m64[sel[t]], at the end mind
    within bound * m64 elementwise.  Returns (the largest share of the bound used by radius / mind,
    the smallest m64[sel[t]] / max(m64))."""
    X = np.asarray(X, dtype=np.float32)
    N, D = X.shape
    b = bound(D)
    sel = np.asarray(sel, dtype=np.int64)
    radius = np.asarray(radius, dtype=np.float32)
    m64 = np.array(mind0, dtype=np.float64)       # the device's fp32 start, or its float64 definition
    assert sel.shape == radius.shape and ((sel >= 0) & (sel < N)).all(), (what, sel)
    share, ratio = 0.0, 1.0
    for t, i in enumerate(sel):
        top, mine = m64.max(), m64[i]
        assert mine >= (1.0 - 2.0 * b) * top, f"{what}: pick {t} = row {i} at {mine}, the farthest " \
                                             f"row is at {top}"
        assert close(radius[t], mine, b), f"{what}: radius[{t}] = {radius[t]}, float64 {mine}"
        if np.isfinite(mine) and mine > 0:
            share = max(share, abs(float(radius[t]) - mine) / (b * mine))
            ratio = min(ratio, mine / top)
        m64 = lower(m64, dist(X, X[i]))
    got = np.asarray(mind, dtype=np.float32)
    ok = close(got, m64, b)
    assert ok.all(), (what, np.nonzero(~ok)[0][:8], got[~ok][:8], m64[~ok][:8])
    assert (got[sel] == 0.0).all(), f"{what}: mind of a chosen row is not exactly 0"
    fin = np.isfinite(m64) & (m64 > 0)
    if fin.any():
        share = max(share, float((np.abs(got[fin] - m64[fin]) / (b * m64[fin])).max()))
    return share, ratio
