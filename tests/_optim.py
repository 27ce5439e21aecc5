"""AdamW and LAMB as include/cilrs_hip.h defines them ("AdamW and LAMB with per-tensor trust
ratios"), stated twice on the CPU for ONE segment (= one parameter tensor) at a time:

  * step64: torch float64 throughout, scalars left in double -- the value the definition means;
  * step32: torch fp32 with the header's operation order, every operation rounded separately (no
    FMA), the scalars rounded to fp32 once, the two norms accumulated and rooted in double -- what
    a device without contraction would compute.

Both take the pre-step p, m, v and the gradient of the segment and return (p, m, v, r): new
parameters and moments and the trust ratio (1.0 for AdamW and under NO_ADAPT).  Inputs are never
modified.  `gs` is the gradient scale as the kernel forms it: float32(clip coefficient) *
float32(grad_scale) in fp32, or grad_scale alone.
"""
import math

import torch

NO_DECAY, NO_ADAPT = 1, 2
ADAMW, LAMB = 1, 2


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def scalars(lr, step, b1, b2):
    """the double-precision scalar preparation of the step entry"""
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    return dict(omb1=1.0 - b1, beta2=b2, omb2=1.0 - b2, inv_bc1=1.0 / bc1,
                neg_step_size=-(lr / bc1), bc2_sqrt=math.sqrt(bc2))


def gscale32(clip_coef, grad_scale):
    """gs as the kernels form it (fp32 product), as a Python float"""
    if clip_coef is None:
        return float(_f32(grad_scale))
    return float(_f32(clip_coef) * _f32(grad_scale))


def _ratio(p_pre, u, flags, trust_clip):
    if flags & NO_ADAPT:
        return 1.0
    np_ = math.sqrt(float((p_pre.double() ** 2).sum()))
    nu = math.sqrt(float((u.double() ** 2).sum()))
    if trust_clip > 0:
        np_ = min(np_, trust_clip)
    return np_ / nu if (np_ > 0.0 and nu > 0.0) else 1.0


def step64(kind, p, g, m, v, *, lr, step, b1, b2, eps, wd, gs=1.0, flags=0, trust_clip=0.0):
    s = scalars(lr, step, b1, b2)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    wd_s = 0.0 if flags & NO_DECAY else wd
    gg = g * gs
    m = m + s["omb1"] * (gg - m)
    v = v * s["beta2"] + (s["omb2"] * gg) * gg
    denom = v.sqrt() / s["bc2_sqrt"] + eps
    if kind == ADAMW:
        p = p * (1.0 - lr * wd_s)
        p = p + (s["neg_step_size"] * m) / denom
        return p, m, v, 1.0
    u = (m * s["inv_bc1"]) / denom + wd_s * p
    r = _ratio(p, u, flags, trust_clip)
    return p - (lr * r) * u, m, v, r


def step32(kind, p, g, m, v, *, lr, step, b1, b2, eps, wd, gs=1.0, flags=0, trust_clip=0.0):
    s = {k: _f32(x) for k, x in scalars(lr, step, b1, b2).items()}
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
    wd_s = _f32(0.0 if flags & NO_DECAY else wd)
    eps32 = _f32(eps)
    gg = g * _f32(gs)
    m = m + s["omb1"] * (gg - m)
    v = v * s["beta2"] + (s["omb2"] * gg) * gg
    denom = v.sqrt() / s["bc2_sqrt"] + eps32
    if kind == ADAMW:
        decay = _f32(1.0 - lr * (0.0 if flags & NO_DECAY else wd))
        p = p * decay
        p = p + (s["neg_step_size"] * m) / denom
        return p, m, v, 1.0
    u = (m * s["inv_bc1"]) / denom + wd_s * p
    r = _ratio(p, u, flags, trust_clip)
    out = p - _f32(lr * r) * u
    assert out.dtype == torch.float32 and m.dtype == torch.float32 and v.dtype == torch.float32
    return out, m, v, r


def gate(name, got, want64, floor32, scale=None):
    """rule of the LAMB tests: max|got - f64| <= 8 * max(max|fp32 restatement - f64|,
    2^-24 * max|f64 value|).  Returns (error, allowed) after asserting."""
    err = float((got.double() - want64).abs().max())
    own = float((floor32.double() - want64).abs().max())
    mag = float(want64.abs().max()) if scale is None else float(scale)
    allowed = 8.0 * max(own, 2.0 ** -24 * mag)
    assert err <= allowed, f"{name}: |device - float64| = {err:.3e} > {allowed:.3e} " \
                           f"(fp32 restatement {own:.3e}, max |value| {mag:.3e})"
    return err, own
