"""The exponential moving average of the weights, restated on the CPU (test_ema_host.py,
test_ema_gpu.py).  The reference keeps no such average: include/cilrs_hip.h states the definition,
this file is its oracle, in fp32 (what the kernels must return bit for bit) and in float64 (what
bounds the fp32 error).

    d_t = min(d, (1 + t) / (10 + t))  with warmup, else d          t = 1-based update count
    w   = float32(1 - d_t)                                         in double, rounded once
    ema = ema + w * (p - ema)                                      three separately rounded fp32 ops

torch.lerp / torch._foreach_lerp_ are NOT this expression (they differ from it by one ulp on the
CPU build), hence the explicit three-operation form: every torch CPU operator below rounds once.
"""
import numpy as np
import torch


def decay_at(d, t, warmup=True):
    """decay of update t (1-based), in double"""
    d = float(d)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def weight32(d, t, warmup=True):
    """w as a Python float that holds an fp32 value exactly"""
    return float(np.float32(1.0 - decay_at(d, t, warmup)))


def step32(ema, p, w):
    """one update in fp32 on CPU tensors; returns the new ema"""
    assert ema.dtype == torch.float32 and p.dtype == torch.float32
    assert ema.device.type == "cpu" and p.device.type == "cpu"
    w32 = torch.tensor(w, dtype=torch.float32)
    assert float(w32) == w, "w must already be an fp32 value"
    diff = p - ema                  # rounding 1
    scaled = diff * w32             # rounding 2
    return ema + scaled             # rounding 3


def step64(ema64, p, w):
    """the same update in float64, fed the fp32 parameters and the fp32 weight"""
    assert ema64.dtype == torch.float64
    return ema64 + float(w) * (p.double() - ema64)


def chain32(ema0, ps, ws):
    """[ema after update 1, 2, ...] in fp32 from the start value and per-step parameters / weights"""
    out, e = [], ema0.clone()
    for p, w in zip(ps, ws):
        e = step32(e, p, w)
        out.append(e)
    return out


def chain64(ema0, ps, ws):
    out, e = [], ema0.double().clone()
    for p, w in zip(ps, ws):
        e = step64(e, p, w)
        out.append(e)
    return out


def running_max(ema0, ps, emas):
    """M after each step: per element the running maximum of max(|ema|, |p|), the start included"""
    out, m = [], ema0.abs().double()
    for p, e in zip(ps, emas):
        m = torch.maximum(m, torch.maximum(p.abs().double(), e.abs().double()))
        out.append(m)
    return out


def bound(T, M):
    """Per-element bound of |fp32 chain - float64 chain| after T updates with every w <= 0.5.
    One update rounds three times: the difference (|p - e| <= 2 M), the product (w |p - e| <= M
    for w <= 0.5) and the sum (|e'| <= M), each to half an ulp, 2^-24 relative: at most
    2^-24 (2 M + M + M) = 4 * 2^-24 * M.  The error carried in from earlier updates is multiplied
    by d_t < 1, so T updates stay within T times that."""
    return 4.0 * T * 2.0 ** -24 * M


def worst_ratio(got32, want64, T, M):
    """max over the elements of |got - want| / bound (0 where the bound is 0 and the error too)"""
    err = (got32.double() - want64).abs()
    b = bound(T, M)
    ok_zero = (b == 0) & (err == 0)
    ratio = torch.where(ok_zero, torch.zeros_like(err), err / b)
    return float(ratio.max())
