"""float64 restatement of the feature-space novelty score (include/cilrs_hip.h, "Feature-space
novelty"; csrc/novelty.hip): the shifted moment table, the finalising algebra and the score, written
independently of cilrs_mi355/novelty.py in numpy."""
import numpy as np


def table_doubles(F, NC):
    return NC * (F + 1) + F * F


def split(table, F, NC):
    """(n [NC], s [NC][F], G [F][F]) views of a flat table"""
    t = np.asarray(table)
    return t[:NC], t[NC:NC + NC * F].reshape(NC, F), t[NC * (F + 1):].reshape(F, F)


def branch(cmd, NC):
    """a command outside 0..NC-1 counts as command 0"""
    c = np.asarray(cmd, dtype=np.int64)
    return np.where((c < 0) | (c >= NC), 0, c)


def relu_features(N, F, NC, seed, dead=0.1, ld=None):
    """Post-ReLU shaped synthetic pooled features: a low-rank mixture plus noise through a ReLU,
    command-dependent offsets, a share `dead` of channels exactly zero.  Returns (v fp32 [N][F],
    cmd int64 [N])."""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(0, NC, size=N)
    rank = 24
    A = rng.standard_normal((rank, F)) / np.sqrt(rank)
    z = rng.standard_normal((N, rank))
    off = rng.standard_normal((NC, F)) * 0.5
    v = np.maximum(z @ A + off[cmd] + 0.3 * rng.standard_normal((N, F)) + 0.4, 0.0)
    v[:, rng.random(F) < dead] = 0.0
    return v.astype(np.float32), cmd.astype(np.int64)


def moments(v, cmd, pivot, NC, table=None):
    """The moment table of rows v (fp32) in float64, added to `table` (a flat float64 array, or
    None for zeros).  Entries j > i of G stay as they were."""
    v = np.asarray(v, dtype=np.float32)
    N, F = v.shape
    t = np.zeros(table_doubles(F, NC)) if table is None else np.array(table, dtype=np.float64)
    n, s, G = split(t, F, NC)
    x = v.astype(np.float64) - np.asarray(pivot, dtype=np.float32).astype(np.float64)[None, :]
    k = branch(cmd, NC)
    for c in range(NC):
        n[c] += float((k == c).sum())
        s[c] += x[k == c].sum(axis=0)
    G += np.tril(x.T @ x)
    return t


def moments_bound(v, pivot, rows=None):
    """rows * 2^-52 * sum_b |x_bi x_bj| [F][F]: the gate of one chain of `rows` fma steps"""
    x = np.abs(np.asarray(v, dtype=np.float32).astype(np.float64)
               - np.asarray(pivot, dtype=np.float32).astype(np.float64)[None, :])
    rows = x.shape[0] if rows is None else rows
    return rows * 2.0 ** -52 * (x.T @ x), rows * 2.0 ** -52 * x


def finalize(table, pivot, F, NC, shrinkage):
    """dict: mean / W (float64), mean32 / W32 (rounded once), sigma, sigma_l, present, N, Kp"""
    n, s, G = split(np.asarray(table, dtype=np.float64), F, NC)
    c = np.asarray(pivot, dtype=np.float32).astype(np.float64)
    low = np.tril(G)
    G = low + np.tril(low, -1).T
    present = n > 0
    N, Kp = n.sum(), int(present.sum())
    Sw = G.copy()
    mean = np.zeros((NC, F))
    for k in range(NC):
        if present[k]:
            m = s[k] / n[k]
            Sw -= n[k] * np.outer(m, m)
            mean[k] = c + m
    sigma = Sw / (N - Kp)
    sigma_l = (1.0 - shrinkage) * sigma + shrinkage * (np.trace(sigma) / F) * np.eye(F)
    Lc = np.linalg.cholesky(sigma_l)
    W = np.tril(np.linalg.solve(Lc, np.eye(F)))
    return dict(mean=mean, W=W, mean32=mean.astype(np.float32), W32=W.astype(np.float32), sigma=sigma,
                sigma_l=sigma_l, L=Lc, present=present, N=int(round(N)), Kp=Kp)


def two_pass(v, cmd, NC):
    """(Sigma, means, present) straight from the definition: class means first, then the pooled
    covariance of the centred rows over N - K'"""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    k = branch(cmd, NC)
    N, F = v.shape
    S = np.zeros((F, F))
    mean = np.zeros((NC, F))
    present = np.zeros(NC, dtype=bool)
    for c in range(NC):
        rows = v[k == c]
        if len(rows):
            present[c] = True
            mean[c] = rows.mean(axis=0)
            d = rows - mean[c]
            S += d.T @ d
    return S / (N - int(present.sum())), mean, present


def score(v, cmd, mean32, W32):
    """d2 [N] in float64 of the ROUNDED fp32 tables, with u = v - mean[k] taken in fp32 as the
    device takes it, and the bound of an fp32 evaluation (tests/test_gradcam_gpu.py's style):
      e_i = (i + 18) 2^-24 sum_j |W_ij||u_j| per row (i + 1 products and their sums, the butterfly),
      sum_i (2 |y_i| e_i + e_i^2) + (F + 16) 2^-24 sum_i y_i^2 for the sum of squares."""
    v = np.asarray(v, dtype=np.float32)
    NC, F = mean32.shape
    u = (v[:, :F] - np.asarray(mean32, dtype=np.float32)[branch(cmd, NC)]).astype(np.float64)
    W = np.tril(np.asarray(W32, dtype=np.float32).astype(np.float64))
    y = u @ W.T
    d2 = (y * y).sum(axis=1)
    e = (np.arange(F) + 18.0)[None, :] * 2.0 ** -24 * (np.abs(u) @ np.abs(W).T)
    bound = (2.0 * np.abs(y) * e + e * e).sum(axis=1) + (F + 16.0) * 2.0 ** -24 * d2
    return d2, bound


def pool_cell_order(fm):
    """AdaptiveAvgPool2d(1,1) of an fp32 map [B][hw][F] as the device takes it: s += map[p] in cell
    order in fp32, then one fp32 division by hw"""
    fm = np.asarray(fm, dtype=np.float32)
    s = np.zeros((fm.shape[0], fm.shape[2]), dtype=np.float32)
    for p in range(fm.shape[1]):
        s = s + fm[:, p, :]
    return s / np.float32(fm.shape[1])
