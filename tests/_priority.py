"""The definition of prioritised sampling (include/cilrs_hip.h "prioritised sampling") in numpy and
Python integers: the fixed-point update, the draw and its importance weights, and the per-sample
loss rows in float64.  Shared by test_priority_host.py and test_priority_gpu.py; touches no GPU."""
import math

import numpy as np

M64 = (1 << 64) - 1
FIXED_ONE = 1 << 20
Q_MAX = (1 << 32) - 1
STRIDE = 0xD1B54A32D192ED03
CHUNK = 1024                      # table entries per chunk sum of the device's draw


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fixed(p):
    """llrint(p * 2^20) clamped to [1, 2^32 - 1]; NaN and everything not below the top take the top"""
    v = float(p) * float(FIXED_ONE)
    if not v < 4294967295.0:
        return Q_MAX
    if not v >= 1.0:
        return 1
    return int(np.rint(v))


def pow_alpha(x, alpha):
    if alpha == 0.0:
        return 1.0
    if alpha == 1.0:
        return float(x)
    if alpha == 0.5:
        return math.sqrt(x)
    return float(np.power(np.float64(x), np.float64(alpha)))


def fill(base, n, pmax=FIXED_ONE):
    """the table before any visit: fixed(base * pmax / 2^20)"""
    scale = float(pmax) / FIXED_ONE
    return np.array([fixed((1.0 if base is None else float(np.float32(base[i]))) * scale)
                     for i in range(n)], dtype=np.uint32)


def update(q, pos, row_loss, base, alpha, eps, pmax):
    """(new table, new running maximum): the highest b of a repeated position writes, positions
    outside [0, n) write nothing"""
    q = np.array(q, dtype=np.uint32, copy=True)
    n = len(q)
    last = {}
    for b, p in enumerate(np.asarray(pos).tolist()):
        if 0 <= p < n:
            last[p] = b
    for p, b in last.items():
        loss = np.float32(row_loss[b])
        if not np.isfinite(loss):
            v = Q_MAX
        else:
            bs = 1.0 if base is None else float(np.float32(base[p]))
            v = fixed(bs * pow_alpha(float(np.float64(loss)) + eps, alpha))
        q[p] = v
        pmax = max(pmax, v)
    return q, pmax


def segments(total, batch):
    """(lo_b, len_b) of the stratified draw"""
    quo, rem = divmod(total, batch)
    return [(quo * b + min(b, rem), quo + (1 if b < rem else 0)) for b in range(batch)]


def targets(total, batch, seed, counter, stratified):
    out = []
    seg = segments(total, batch) if stratified and total >= batch else None
    for b in range(batch):
        r = splitmix64((seed + ((counter * batch + b) & M64) * STRIDE) & M64)
        if seg is not None:
            lo, ln = seg[b]
            out.append(lo + ((r * ln) >> 64))
        else:
            out.append((r * total) >> 64)
    return out


def draw(q, batch, seed, counter, stratified, beta, subset=None, cum=None):
    """(pos int64 [batch], index int64 [batch], weight float32 [batch]); cum: np.cumsum of the
    table as uint64, when the caller has it already"""
    q = np.asarray(q, dtype=np.uint32)
    if cum is None:
        cum = np.cumsum(q.astype(np.uint64), dtype=np.uint64)
    total = int(cum[-1])
    t = np.array(targets(total, batch, seed, counter, stratified), dtype=np.uint64)
    pos = np.searchsorted(cum, t, side="right").astype(np.int64)
    index = pos if subset is None else np.asarray(subset, dtype=np.int64)[pos]
    v = np.power(np.float64(total) / (np.float64(len(q)) * q[pos].astype(np.float64)),
                 np.float64(beta))
    weight = (v / v.max()).astype(np.float32)
    return pos, index, weight


def loss_rows(pc, tc, ps, ts, kind, w4):
    """float64 row terms l_b from the fp32 differences (numpy float32 arrays in)"""
    d = (np.asarray(pc, np.float32) - np.asarray(tc, np.float32)).astype(np.float64)
    ds = (np.asarray(ps, np.float32) - np.asarray(ts, np.float32)).astype(np.float64)
    w = [float(np.float32(x)) for x in w4]
    if kind == 0:
        row = ((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2) / 3.0
    else:
        row = (w[0] * np.abs(d[:, 0]) + w[1] * np.abs(d[:, 1])) + w[2] * np.abs(d[:, 2])
    return row + w[3] * ds ** 2
