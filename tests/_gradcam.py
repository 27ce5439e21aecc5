"""Grad-CAM of a trunk group: the definition the engine is held to (include/cilrs_hip.h,
cilrs_net_gradcam), restated in float64 -- shared by tests/test_gradcam_host.py and
tests/test_gradcam_gpu.py.  The reference has no such path; parity is pinned by this definition.

Per frame, with w the four output weights and y = w . (steer, throttle, brake, pred_speed) on the
raw eval-mode outputs of the commanded branch (a command outside 0..NC-1: branch 0):
  A        post-ReLU output of trunk group L, NHWC [h][w][C]
  dA       dy / dA; for layer4 dA[c,i,j] = g[c] / (h*w), g = dy / d pooled from the heads alone
           (branch part + speed-predictor part, in that order)
  alpha[c] = (1/(h*w)) sum_ij dA[c,i,j]
  cam[i,j] = sum_c alpha[c] A[c,i,j]                     (signed)
  peak     = max_ij max(cam, 0);  n = max(cam, 0) / peak, 0 everywhere when peak == 0
  heat     = bilinear interpolation of n to [H][W], half-pixel centres: source coordinate
             (y + 0.5) * h / H - 0.5 clamped to [0, h-1], upper neighbour clamped to h-1
  heat_u8  = floor(heat * 255 + 0.5) in fp32
"""
import numpy as np
import torch
import torch.nn as nn

U = 2.0 ** -24              # unit roundoff of fp32
TOL_OUT = 2e-5              # the four outputs against float64: the MC tests' gate (_mc_dropout.TOL)
TOL_HEAT = 1e-6             # heat against the float64 interpolation of the device's own n
MARGIN = 1e-4               # no head pre-activation of a test's inputs may lie this close to zero


def _linears(seq):
    return [(m.weight.detach().double(), m.bias.detach().double()) for m in seq
            if isinstance(m, nn.Linear)]


def heads_input_grad64(model, pooled, speed, command, weights4):
    """float64 heads forward and backward on pooled features [B, F].  Returns a dict:
    g [B, F] = d (w . outputs) / d pooled; out [B, 4]; S [B, F], the sum of absolute products along
    the chain that gives g (the forward-error scale of its fp32 evaluation under the same ReLU
    decisions); margin, the smallest |pre-activation| of any head unit."""
    nc = len(model.control_branches)
    se, sp = _linears(model.speed_encoder), _linears(model.speed_predictor)
    w = torch.as_tensor(np.asarray(weights4, dtype=np.float64))
    v = pooled.double()
    B, F = v.shape
    g, S, out = torch.zeros(B, F, dtype=torch.float64), torch.zeros(B, F, dtype=torch.float64), \
        torch.zeros(B, 4, dtype=torch.float64)
    margin = float("inf")
    for b in range(B):
        k = int(command[b]) if 0 <= int(command[b]) < nc else 0
        br = _linears(model.control_branches[k])
        x = speed[b].double().view(1)
        za = se[0][0] @ x + se[0][1]
        zf = se[1][0] @ za.clamp(min=0) + se[1][1]
        comb = torch.cat([v[b], zf.clamp(min=0)])
        z1 = br[0][0] @ comb + br[0][1]
        z2 = br[1][0] @ z1.clamp(min=0) + br[1][1]
        out[b, :3] = br[2][0] @ z2.clamp(min=0) + br[2][1]
        q1 = sp[0][0] @ v[b] + sp[0][1]
        q2 = sp[1][0] @ q1.clamp(min=0) + sp[1][1]
        out[b, 3] = (sp[2][0] @ q2.clamp(min=0) + sp[2][1])[0]
        margin = min(margin, *(float(z.abs().min()) for z in (za, zf, z1, z2, q1, q2)))
        # the branch
        dh2 = (br[2][0].t() @ w[:3]) * (z2 > 0)
        dh1 = (br[1][0].t() @ dh2) * (z1 > 0)
        gb = br[0][0][:, :F].t() @ dh1
        sh2 = (br[2][0].abs().t() @ w[:3].abs()) * (z2 > 0)
        sh1 = (br[1][0].abs().t() @ sh2) * (z1 > 0)
        sb = br[0][0][:, :F].abs().t() @ sh1
        # the speed predictor
        dp2 = (sp[2][0].t() @ w[3:]) * (q2 > 0)
        dp1 = (sp[1][0].t() @ dp2) * (q1 > 0)
        gs = sp[0][0].t() @ dp1
        sp2 = (sp[2][0].abs().t() @ w[3:].abs()) * (q2 > 0)
        sp1 = (sp[1][0].abs().t() @ sp2) * (q1 > 0)
        ss = sp[0][0].abs().t() @ sp1
        g[b] = gb + gs
        S[b] = sb + ss
    return dict(g=g, out=out, S=S, margin=margin)


def g_bound(S, feat):
    """|g - g64| <= (K + 16) * 2^-24 * S per element, K the longest dot product of the chain
    (the branch's first layer: feat + 128 = 640, or 2176 for the wide trunk)"""
    return (feat + 128 + 16) * U * S


def source_index(n_out, n_in):
    """(lower neighbour, upper neighbour, weight of the upper) per output index: half-pixel centres,
    the source coordinate clamped to [0, n_in - 1], in float64"""
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5
    s = np.clip(s, 0.0, float(n_in - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def upsample64(n, H, W):
    """bilinear interpolation of n [B, h, w] to float64 [B, H, W]"""
    n = np.asarray(n, dtype=np.float64)
    y0, y1, ly = source_index(H, n.shape[1])
    x0, x1, lx = source_index(W, n.shape[2])
    top = n[:, y0][:, :, x0] * (1.0 - lx) + n[:, y0][:, :, x1] * lx
    bot = n[:, y1][:, :, x0] * (1.0 - lx) + n[:, y1][:, :, x1] * lx
    return top * (1.0 - ly)[None, :, None] + bot * ly[None, :, None]


def normalise64(cam):
    """(max(cam, 0) / peak with 0 for peak == 0, peak) of cam [B, h, w], float64"""
    pos = np.maximum(np.asarray(cam, dtype=np.float64), 0.0)
    peak = pos.reshape(pos.shape[0], -1).max(axis=1)
    safe = np.where(peak > 0.0, peak, 1.0)
    return np.where(peak[:, None, None] > 0.0, pos / safe[:, None, None], 0.0), peak


def gradcam64(A, H, W, dA=None, g=None):
    """The definition on A [B, h, w, C]: dict(alpha [B, C], cam [B, h, w], peak [B], n, heat
    [B, H, W], cam_scale [B, h, w] = sum_c abar_c |A_cij| with abar_c = (1/(h*w)) sum_ij |dA_cij|)."""
    assert (dA is None) != (g is None)
    A = np.asarray(A, dtype=np.float64)
    B, h, w, C = A.shape
    if dA is not None:
        dA = np.asarray(dA, dtype=np.float64)
        alpha = dA.reshape(B, h * w, C).sum(axis=1) / (h * w)
        abar = np.abs(dA).reshape(B, h * w, C).sum(axis=1) / (h * w)
    else:
        alpha = np.asarray(g, dtype=np.float64) / (h * w)
        abar = np.abs(alpha)
    cam = (A * alpha[:, None, None, :]).sum(axis=3)
    n, peak = normalise64(cam)
    return dict(alpha=alpha, cam=cam, peak=peak, n=n, heat=upsample64(n, H, W),
                cam_scale=(np.abs(A) * abar[:, None, None, :]).sum(axis=3))


def cam_bound(cam_scale, C, hw):
    """|cam - cam64| <= (C + h*w + 16) * 2^-24 * sum_c abar_c |A_cij| per element: a dot product of
    C terms whose weights are sums of h*w terms"""
    return (C + hw + 16) * U * cam_scale


def heat_u8_of(heat32):
    """floor(heat * 255 + 0.5) in fp32, from fp32 heat"""
    h = np.asarray(heat32, dtype=np.float32)
    return np.floor(h * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def autograd_gradcam_layers(model, image, speed, command, weights4, layers):
    """torch.autograd Grad-CAM of trunk groups `layers` (each 1..4) of a CILRSOracle-like module in
    one pass, in the module's dtype, eval mode, with a hook on each group's output:
    ({layer: (A [B, h, w, C], dA, cam [B, h, w])}, out [B, 4])."""
    model.eval()
    kept, hooks = {}, []
    for layer in layers:
        def hook(_m, _i, o, layer=layer):
            o.retain_grad()
            kept[layer] = o
        hooks.append(model.visual_encoder[3 + layer].register_forward_hook(hook))
    try:
        ctrl, ps = model(image, speed, command)
    finally:
        for h in hooks:
            h.remove()
    w = torch.as_tensor(np.asarray(weights4), dtype=ctrl.dtype)
    out = torch.cat([ctrl, ps.unsqueeze(1)], dim=1)
    (out * w).sum().backward()
    res = {}
    for layer in layers:
        A, dA = kept[layer].detach(), kept[layer].grad.detach()
        cam = (A * dA.mean(dim=(2, 3))[:, :, None, None]).sum(dim=1)
        res[layer] = (A.permute(0, 2, 3, 1).contiguous(), dA.permute(0, 2, 3, 1).contiguous(), cam)
    return res, out.detach()


def autograd_gradcam(model, image, speed, command, weights4, layer):
    """One group of autograd_gradcam_layers: (A, dA, cam, out)."""
    res, out = autograd_gradcam_layers(model, image, speed, command, weights4, (layer,))
    return res[layer] + (out,)
