"""CPU definition of the 16-bit INFERENCE mode (cilrs_net_forward_u8_f16 / _bf16) -- TEST
INFRASTRUCTURE ONLY.

Not a restatement of reference code: the reference runs its eval forward in fp32
(model/autonomous_drive.py:389-399 under model.eval()) and has no 16-bit path.  This file DEFINES
what the fp16 / bf16 trunk computes, restated from this repository's own kernels, so that they can
be held to one rounding each instead of to a loose "close to fp32" bound.  Parity for this mode is
"parity unpinned" by the reference.

The mode, with T = fp16 or bf16 and round_T = round-to-nearest-even into T:

* fold (fold_bn_f16_kernel, fold_stem_kernel; the scale/shift table of bn_eval_stats_all_kernel):
  rstd = 1 / sqrt(running_var + 1e-5), scale = gamma * rstd, w16 = round_T(w * scale[co]) with the
  product in fp32, bias = beta - running_mean * scale kept in fp32;
* stem (stem_f16_kernel): the fp32 normalised image is rounded to T, convolved 7x7 / stride 2 /
  pad 3 with the folded weights (fp32 accumulation), + bias, ReLU, ONE rounding to T; the max-pool
  3x3 / stride 2 / pad 1 takes maxima of the stored values (exact);
* every trunk convolution, BasicBlock and Bottleneck alike (conv_f16_kernel's inference epilogue):
  y = round_T(relu?((acc + bias) + residual)), acc = the sum of the products of the stored 16-bit
  operands, residual = the stored block input or the stored output of the down-sample
  convolution.  conv1 (and a Bottleneck's conv2) have ReLU and no residual, the down-sample
  convolution has neither, the block's last convolution has both;
* the average pool sums the stored last tensor in fp32 and divides by the pixel count; the heads are
  the fp32 oracle unchanged.

Freedom left to an implementation: the ORDER of each fp32 sum (the kernels accumulate on
v_mfma_f32_32x32x16_*; torch's CPU convolution sums in another order).  `acc` selects the
accumulation type of this emulation: torch.float32 is one more realisation of the mode,
torch.float64 its (practically) order-free value.  The single-step functions take GIVEN stored
inputs and return the value BEFORE the final rounding, which is what the layer-by-layer GPU tests
compare a kernel's stored result with.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
# significant bits p and the smallest spacing (exponent of two) of the two 16-bit formats
_FORMAT = {torch.float16: (11, -24), torch.bfloat16: (8, -133)}


def is_rounded(T) -> bool:
    return T in _FORMAT


def round_to(t: torch.Tensor, T) -> torch.Tensor:
    """round_T(t), returned in t's own dtype.  T = torch.float32 / float64 switches the rounding
    off.  A float64 input is rounded DIRECTLY (not through fp32, which would round twice: one
    fp32 value in 2^13 is an fp16 tie)."""
    if not is_rounded(T):
        return t
    if t.dtype != torch.float64:
        return t.to(T).to(t.dtype)
    p, emin = _FORMAT[T]
    _, e = torch.frexp(t)                                   # |t| in [2^(e-1), 2^e)
    q = torch.ldexp(torch.ones_like(t), torch.clamp(e - p, min=emin))
    return torch.round(t / q) * q                           # power-of-two scaling is exact; half-even


def half_spacing(ref: torch.Tensor, T) -> torch.Tensor:
    """h(ref) = 2^(floor(log2 |ref|) - p): half the spacing of T in ref's binade (0 at ref == 0)."""
    p, _ = _FORMAT[T]
    _, e = torch.frexp(ref)
    h = torch.ldexp(torch.ones_like(ref), e - 1 - p)
    return torch.where(ref == 0, torch.zeros_like(ref), h)


# ---- single steps on given stored inputs ---------------------------------------------------------
def fold_scale_shift(gamma, beta, running_mean, running_var):
    """The eval-mode BatchNorm table in fp32: (scale, shift) = (gamma * rstd, beta - mean * scale)."""
    one = torch.ones((), dtype=torch.float32)
    rstd = one / torch.sqrt(running_var.float() + torch.tensor(BN_EPS, dtype=torch.float32))
    scale = gamma.float() * rstd
    return scale, beta.float() - running_mean.float() * scale


def fold_conv_bn(w, gamma, beta, running_mean, running_var, T):
    """(w16, bias) of one convolution / BatchNorm pair: w OIHW fp32 -> folded OIHW weights holding
    values of T (as fp32 numbers; unrounded when T is a float type), bias fp32."""
    scale, shift = fold_scale_shift(gamma, beta, running_mean, running_var)
    return round_to(w.float() * scale.view(-1, 1, 1, 1), T), shift


def fold_conv_bn_ref64(w, gamma, running_var):
    """float64 value of the folded weights BEFORE the rounding."""
    return w.double() * (gamma.double() / torch.sqrt(running_var.double() + BN_EPS)).view(-1, 1, 1, 1)


def conv_pre(x, w16, bias, residual=None, relu=True, stride=1, pad=0, acc=torch.float64):
    """One trunk convolution on stored operands, BEFORE the final rounding:
    relu?((conv(x, w16) + bias) + residual) in `acc` arithmetic.  x, residual NCHW, w16 OIHW."""
    y = F.conv2d(x.to(acc), w16.to(acc), None, stride, pad) + bias.to(acc).view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.to(acc)
    return F.relu(y) if relu else y


def stem_pre(image, w16, bias, T, acc=torch.float64):
    """The stem on the fp32 normalised image [N,3,H,W] and the folded OIHW [64,3,7,7] weights,
    BEFORE the final rounding: relu(conv7x7/s2/p3(round_T(image), w16) + bias)."""
    return conv_pre(round_to(image.float(), T), w16, bias, None, True, 2, 3, acc)


def maxpool(x):
    return F.max_pool2d(x, 3, 2, 1)


def avgpool(x, acc=torch.float64):
    """[N,C,H,W] stored tensor -> [N,C] mean in `acc` arithmetic."""
    n, c = x.shape[:2]
    return x.to(acc).reshape(n, c, -1).sum(-1) / float(x.shape[2] * x.shape[3])


# ---- the network ---------------------------------------------------------------------------------
def block_convs(blk):
    """[(conv, bn)] of a BasicBlock / Bottleneck main branch, and its down-sample pair or None."""
    pairs = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
    if hasattr(blk, "conv3"):
        pairs.append((blk.conv3, blk.bn3))
    down = None if blk.downsample is None else (blk.downsample[0], blk.downsample[1])
    return pairs, down


def trunk_blocks(model):
    """The residual blocks of visual_encoder.{4..7} in order (both oracles share the wrapping)."""
    return [blk for li in (4, 5, 6, 7) for blk in model.visual_encoder[li]]


def _fold(conv, bn, T):
    return fold_conv_bn(conv.weight.detach(), bn.weight.detach(), bn.bias.detach(),
                        bn.running_mean, bn.running_var, T)


@torch.no_grad()
def features(model, image, T, acc=torch.float32):
    """Pooled trunk features [N, feat] of the mode (dtype `acc`), for CILRSOracle and the ResNet-50
    oracle.  T = torch.float16 / bfloat16; torch.float32 / float64 = no rounding anywhere."""
    ve = model.visual_encoder
    w, b = _fold(ve[0], ve[1], T)
    x = round_to(stem_pre(image, w, b, T, acc), T)
    x = maxpool(x)
    for blk in trunk_blocks(model):
        pairs, down = block_convs(blk)
        identity = x
        if down is not None:
            w, b = _fold(down[0], down[1], T)
            identity = round_to(conv_pre(x, w, b, None, False, down[0].stride[0], 0, acc), T)
        out = x
        for i, (conv, bn) in enumerate(pairs):
            w, b = _fold(conv, bn, T)
            last = i + 1 == len(pairs)
            out = round_to(conv_pre(out, w, b, identity if last else None, True, conv.stride[0],
                                    conv.padding[0], acc), T)
        x = out
    return avgpool(x, acc)


@torch.no_grad()
def heads(model, visual, speed, command):
    """The fp32 heads of the oracle (CILRSOracle.forward after the visual encoder)."""
    visual = visual.float()
    speed_feat = model.speed_encoder(speed.unsqueeze(1))
    combined = torch.cat([visual, speed_feat], dim=1)
    pred_speed = model.speed_predictor(visual).squeeze(1)
    b = visual.size(0)
    all_out = torch.stack([br(combined) for br in model.control_branches], dim=0)
    idx = command.unsqueeze(0).unsqueeze(2).expand(1, b, 3)
    return all_out.gather(0, idx).squeeze(0), pred_speed


@torch.no_grad()
def forward(model, image, speed, command, T, acc=torch.float32):
    """(controls, pred_speed) of the whole mode; the model must be in eval mode."""
    assert not model.training, "the 16-bit inference mode folds the RUNNING statistics"
    return heads(model, features(model, image, T, acc), speed, command)


def perturbed_state_dict(sd, seed=0):
    """A copy of a CILRS state dict whose trunk BatchNorm layers are pushed away from the portable
    initialisation, so that no two layers (or channels) fold alike: running_var log-uniform in
    [1e-3, 1e2], gamma of both signs scaled so that gamma * rstd keeps its magnitude (activations
    stay O(1)), running_mean and beta moved.  Deterministic in (seed, key order)."""
    out = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sd:
        if not (k.startswith("visual_encoder") and k.endswith("running_var")):
            continue
        base = k[:-len("running_var")]
        c = sd[k].numel()
        var = 10.0 ** (torch.rand(c, generator=g) * 5.0 - 3.0)
        sign = torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
        old_scale = sd[base + "weight"] / torch.sqrt(sd[k] + BN_EPS)
        out[k] = var
        out[base + "weight"] = sign * old_scale * (0.8 + 0.4 * torch.rand(c, generator=g)) * \
            torch.sqrt(var + BN_EPS)
        out[base + "running_mean"] = sd[base + "running_mean"] + 0.1 * torch.randn(c, generator=g)
        out[base + "bias"] = sd[base + "bias"] + 0.1 * torch.randn(c, generator=g)
    return out
