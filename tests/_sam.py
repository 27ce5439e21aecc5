"""The SAM / ASAM perturbation as include/cilrs_hip.h defines it ("sharpness-aware minimisation"),
stated twice on the CPU over one flat range:

  * perturb64: torch float64 throughout -- the value the definition means.  The adaptive t is the
    header's fp32 product |p| * g (its one rounding is part of the definition of S).
  * perturb32: torch fp32 with the header's operation order, every operation rounded separately (no
    FMA) -- what a device without contraction computes, bit for bit.  It takes s32, the fp32 scale,
    as an argument: the norm is a double-precision quantity and has no fp32 restatement.

Inputs are never modified.
"""
import math

import numpy as np
import torch

NORM_EPS = 1e-12


def t32(p, g, adaptive):
    """t of the definition, fp32: g, or |p| * g rounded once"""
    assert p.dtype == g.dtype == torch.float32
    return p.abs() * g if adaptive else g


def norm_scale(p, g, rho, adaptive):
    """(S, norm, scale) in double; S = math.fsum of the float64 squares (exactly rounded)"""
    t = t32(p, g, adaptive).double()
    S = math.fsum((t * t).tolist())
    norm = math.sqrt(S)
    return S, norm, rho / (norm + NORM_EPS)


def s32_of(scale):
    """(float)scale: one rounding of the double to fp32, as a Python float"""
    with np.errstate(over="ignore"):
        return float(np.float32(scale))


def perturb64(p, g, rho, adaptive):
    """-> (new p in float64, S, norm, scale)"""
    S, norm, scale = norm_scale(p, g, rho, adaptive)
    pd, gd = p.double(), g.double()
    if adaptive:
        return pd + scale * (pd.abs() * (pd.abs() * gd)), S, norm, scale
    return pd + scale * gd, S, norm, scale


def perturb32(p, g, s32, adaptive):
    """-> new p in fp32: p + s32 * g (two roundings) or p + s32 * (|p| * (|p| * g)) (four, the first
    of them t's)"""
    assert p.dtype == g.dtype == torch.float32
    s = torch.tensor(float(s32), dtype=torch.float32)
    assert float(s) == float(s32), "s32 must be an fp32 value"
    if adaptive:
        a = p.abs()
        t = a * g
        d = a * t
    else:
        d = g
    step = s * d
    out = p + step
    assert out.dtype == torch.float32
    return out
