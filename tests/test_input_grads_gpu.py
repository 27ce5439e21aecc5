"""Gradients with respect to the INPUTS of the HIP engine (image.grad / speed.grad, autograd.grad)
in train mode and -- through the frozen-BatchNorm forward -- in eval mode, and the stem's
data-gradient kernel behind them (include/cilrs_hip.h: cilrs_net_forward_frozen,
cilrs_net_input_grads, cilrs_stem_conv_dgrad).

Gates, built like tests/test_model_gpu.py's:
  stem dgrad (op)   element-wise <= 1e-5 * max|dx| against torch.nn.grad.conv2d_input in float64;
                    two runs bit-identical
  input gradients   relative L2 error against a float64 run of the same graph <= max(4x the fp32
                    CPU oracle's own error, 5e-3); 1 - cosine <= max(4x the CPU oracle's, 1e-5)
  parameter grads   per tensor the same relative-L2 gate, cosine of the whole gradient
                    >= 1 - 2.5e-5 (the floor test_model_gpu.py uses at small batches)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cilrs_oracle as O

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4


def make_model(seed=0, dropout=0.0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=dropout)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda()


def to_dev(*ts):
    return [t.cuda() for t in ts]


def _loss(pc, ps, tgt, spd):
    return O.compute_loss(O.CONFIG_A, pc, tgt, ps, spd)[0]


def _rel(a, ref):
    return float((a.double() - ref).norm()) / max(float(ref.norm()), 1e-30)


def _cos(a, ref):
    a = a.double().flatten()
    ref = ref.flatten()
    return float((a * ref).sum()) / max(float(a.norm() * ref.norm()), 1e-300)


def _check_input_grad(tag, mine, cpu32, ref64):
    mine = mine.detach().cpu()
    e_gpu, e_cpu = _rel(mine, ref64), _rel(cpu32, ref64)
    cos, cos_cpu = _cos(mine, ref64), _cos(cpu32, ref64)
    print(f"{tag}: relative L2 vs float64 {e_gpu:.3e} (fp32 CPU oracle {e_cpu:.3e}), 1-cos "
          f"{1 - cos:.3e} (CPU {1 - cos_cpu:.3e})")
    assert e_gpu <= max(4.0 * e_cpu, 5e-3), (tag, e_gpu, e_cpu)
    # (a noisier graph -- half the head units dropped at B = 16 -- puts the fp32 CPU oracle itself
    #  at 1 - cos ~ 1e-5: the floor is then a small multiple of its own, as in test_model_gpu.py)
    assert 1.0 - cos <= max(4.0 * (1.0 - cos_cpu), 1e-5), (tag, 1.0 - cos, 1.0 - cos_cpu)


def _oracle_grads(build, mode, imgs, spds, cmds, tgts, dtype, masks=None):
    """(image.grad, speed.grad, {name: param.grad}, outputs) of the oracle in `dtype`."""
    m = build(0).to(dtype)
    m.train() if mode == "train" else m.eval()
    x = imgs.detach().clone().to(dtype).requires_grad_()      # (new leaves: never the callers'
    v = spds.detach().clone().to(dtype).requires_grad_()      #  tensors, whatever dtype)
    if masks is None:
        pc, ps = m(x, v, cmds)
    else:
        pc, ps = O.forward_with_dropout_masks(m, x, v, cmds, {k: t.to(dtype) for k, t in masks.items()})
    _loss(pc, ps, tgts.to(dtype), spds.to(dtype)).backward()
    return x.grad, v.grad, {n: p.grad for n, p in m.named_parameters()}, (pc.detach(), ps.detach())


# ---- the stem's data gradient, op level ---------------------------------------------------------
def _stem_dgrad(dy_nhwc, w_ohwi, dx):
    from cilrs_mi355 import _lib as L
    n, _, h, w = dx.shape
    L.check(L.lib().cilrs_stem_conv_dgrad(L.ptr(dy_nhwc), L.ptr(w_ohwi), L.ptr(dx), *dx.stride(),
                                          n, h, w, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,H,W", [(2, 88, 200), (1, 176, 400), (2, 90, 202), (3, 96, 160),
                                   (1, 64, 64), (1, 37, 51)])
@pytest.mark.parametrize("channels_last", [False, True])
def test_stem_dgrad_matches_conv2d_input(N, H, W, channels_last):
    g = torch.Generator().manual_seed(N * 1000 + H + W)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(N, ho, wo, 64, generator=g)
    w = torch.randn(64, 7, 7, 3, generator=g) * 0.1
    want = torch.nn.grad.conv2d_input((N, 3, H, W), w.permute(0, 3, 1, 2).double(),
                                      dy.permute(0, 3, 1, 2).double(), stride=2, padding=3)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    outs = []
    for _ in range(2):
        dx = torch.full((N, 3, H, W), float("nan"), device="cuda").contiguous(memory_format=fmt)
        _stem_dgrad(dy.cuda(), w.cuda(), dx)
        outs.append(dx)
    assert torch.equal(outs[0], outs[1])                       # no atomics: bit-identical
    got = outs[0].cpu().double()
    assert torch.isfinite(got).all()                           # every element written
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), (err, float(want.abs().max()))


# ---- train mode ---------------------------------------------------------------------------------
def test_train_mode_input_grads_vs_float64_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "forward_train_b8.npz"))
    imgs, spds, cmds, tgts = O.synthetic_batch(8, seed=int(g["seed"]))[:4]
    m = make_model().train()
    params = list(m.parameters())
    # the same step with inputs that do not require grad: the parameter gradients to match
    m.zero_grad(set_to_none=True)
    x, v, c, t = to_dev(imgs, spds, cmds, tgts)
    pc, ps = m(x, v, c)
    _loss(pc, ps, t, v).backward()
    ref_param = [p.grad.detach().clone() for p in params]
    m.zero_grad(set_to_none=True)
    x = imgs.cuda().requires_grad_()
    vg = spds.cuda().requires_grad_()
    pc, ps = m(x, vg, c)
    assert np.abs(pc.detach().cpu().numpy() - g["controls"]).max() <= TOL_OUT
    _loss(pc, ps, t, spds.cuda()).backward()
    for p, r in zip(params, ref_param):
        assert torch.equal(p.grad, r)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    assert vg.grad is not None and vg.grad.shape == vg.shape
    gi64, gs64, _, _ = _oracle_grads(O.build_oracle, "train", imgs, spds, cmds, tgts, torch.float64)
    gi32, gs32, _, _ = _oracle_grads(O.build_oracle, "train", imgs, spds, cmds, tgts, torch.float32)
    _check_input_grad("train image.grad", x.grad, gi32, gi64)
    _check_input_grad("train speed.grad", vg.grad, gs32, gs64)
    # bit-reproducible
    x2 = imgs.cuda().requires_grad_()
    v2 = spds.cuda().requires_grad_()
    pc, ps = m(x2, v2, c)
    _loss(pc, ps, t, spds.cuda()).backward()
    assert torch.equal(x2.grad, x.grad) and torch.equal(v2.grad, vg.grad)


def test_train_mode_speed_grad_under_dropout_masks():
    """dropout 0.5: the masks the kernels applied are regenerated through cilrs_dropout (as
    tests/test_model_gpu.py does) and given to the float64 oracle."""
    from cilrs_mi355 import _lib as L
    B, p, seed = 16, 0.5, 12345
    imgs, spds, cmds, tgts = O.synthetic_batch(B, seed=91)[:4]
    m = make_model(dropout=p).train()
    x = imgs.cuda().requires_grad_()
    v = spds.cuda().requires_grad_()
    c, t = to_dev(cmds, tgts)
    pc, ps = m.engine().forward(x, v, c, True, p, seed)
    _loss(pc, ps, t, spds.cuda()).backward()
    widths = {0: 128, 9: 256, **{s: 256 for s in range(1, 9)}}
    masks = {}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for site, cols in widths.items():
        mk = torch.ones(B, cols, device="cuda")
        L.check(L.lib().cilrs_dropout(L.ptr(mk), B, cols, cols, p, seed, site, st))
        masks[site] = mk.cpu()
    torch.cuda.synchronize()
    assert float((masks[0] == 0).float().mean()) > 0.3
    gi64, gs64, _, (oc, _) = _oracle_grads(O.build_oracle, "train", imgs, spds, cmds, tgts,
                                           torch.float64, masks)
    gi32, gs32, _, _ = _oracle_grads(O.build_oracle, "train", imgs, spds, cmds, tgts,
                                     torch.float32, masks)
    assert float((pc.detach().cpu().double() - oc).abs().max()) <= TOL_OUT
    _check_input_grad("dropout speed.grad", v.grad, gs32, gs64)
    _check_input_grad("dropout image.grad", x.grad, gi32, gi64)


# ---- eval mode (frozen BatchNorm) ---------------------------------------------------------------
def test_eval_mode_graph_vs_float64_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "forward_eval_b4.npz"))
    imgs, spds, _, tgts = O.synthetic_batch(4, seed=int(g["seed"]))[:4]
    cmds = torch.from_numpy(g["command"])
    m = make_model().eval()
    eng = m.engine()
    bn_before, nbt_before = eng.bn.clone(), eng.nbt.clone()
    x = imgs.cuda().requires_grad_()
    v = spds.cuda().requires_grad_()
    c, t = to_dev(cmds, tgts)
    pc, ps = m(x, v, c)
    assert pc.requires_grad and ps.requires_grad
    assert np.abs(pc.detach().cpu().numpy() - g["controls"]).max() <= TOL_OUT
    assert np.abs(ps.detach().cpu().numpy() - g["pred_speed"]).max() <= TOL_OUT
    m.zero_grad(set_to_none=True)
    _loss(pc, ps, t, spds.cuda()).backward()
    torch.cuda.synchronize()
    assert torch.equal(eng.bn, bn_before) and torch.equal(eng.nbt, nbt_before)
    gi64, gs64, gp64, _ = _oracle_grads(O.build_oracle, "eval", imgs, spds, cmds, tgts, torch.float64)
    gi32, gs32, gp32, _ = _oracle_grads(O.build_oracle, "eval", imgs, spds, cmds, tgts, torch.float32)
    _check_input_grad("eval image.grad", x.grad, gi32, gi64)
    _check_input_grad("eval speed.grad", v.grad, gs32, gs64)
    dot = n1 = n2 = 0.0
    for n, p in m.named_parameters():
        mine, ref = p.grad.detach().cpu().double(), gp64[n]
        e_gpu, e_cpu = _rel(mine, ref), _rel(gp32[n], ref)
        assert e_gpu <= max(4.0 * e_cpu, 5e-3), (n, e_gpu, e_cpu)
        dot += float((mine * ref).sum())
        n1 += float((mine ** 2).sum())
        n2 += float((ref ** 2).sum())
    assert 1.0 - dot / (n1 * n2) ** 0.5 <= 2.5e-5
    # torch.autograd.grad with frozen parameters: the same image gradient, bit for bit
    image_grad = x.grad.clone()
    m.requires_grad_(False)
    x2 = imgs.cuda().requires_grad_()
    pc, ps = m(x2, spds.cuda(), c)
    (gx,) = torch.autograd.grad(_loss(pc, ps, t, spds.cuda()), x2)
    assert torch.equal(gx, image_grad)
    torch.cuda.synchronize()
    assert torch.equal(eng.bn, bn_before) and torch.equal(eng.nbt, nbt_before)
    # a later graph forward of the same shape overwrites the saved activations: backward raises
    pc, ps = m(x2, spds.cuda(), c)
    m(imgs.cuda().requires_grad_(), spds.cuda(), c)
    with pytest.raises(RuntimeError, match="overwritten"):
        pc.sum().backward()


def test_eval_mode_channels_last_image_and_detached_fast_path():
    imgs, spds, cmds, _ = O.synthetic_batch(2, seed=5)[:4]
    m = make_model().eval()
    with torch.no_grad():
        want_c, _ = m(*to_dev(imgs, spds, cmds))
    x = imgs.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    pc, _ = m(x, spds.cuda(), cmds.cuda())
    assert (pc.detach() - want_c).abs().max() <= TOL_OUT
    pc[:, 0].sum().backward()
    x_ref = imgs.cuda().requires_grad_()
    pr, _ = m(x_ref, spds.cuda(), cmds.cuda())
    pr[:, 0].sum().backward()
    assert x.grad.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(x.grad, x_ref.grad)
    # nothing asks for a gradient: the eval forward stays detached
    c, s = m(*to_dev(imgs, spds, cmds))
    assert not c.requires_grad and not s.requires_grad


def test_bf16_training_plan_rejects_the_frozen_mode():
    imgs, spds, cmds, _ = O.synthetic_batch(2, seed=5)[:4]
    m = make_model().eval()
    m.engine().train_precision = "bf16"
    with pytest.raises(RuntimeError, match="frozen"):
        m(imgs.cuda().requires_grad_(), spds.cuda(), cmds.cuda())


def test_resnet50_variant_image_grad_vs_its_oracle():
    import resnet50_oracle as R
    from cilrs_mi355 import CILRSResNet50
    B, H, W = 2, 64, 96
    imgs, spds, cmds, tgts = O.synthetic_batch(B, seed=31, h=H, w=W)[:4]
    m = CILRSResNet50(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    m = m.cuda().eval()
    x = imgs.cuda().requires_grad_()
    pc, ps = m(x, spds.cuda(), cmds.cuda())
    _loss(pc, ps, tgts.cuda(), spds.cuda()).backward()
    gi64, _, _, (oc, _) = _oracle_grads(R.build_oracle50, "eval", imgs, spds, cmds, tgts, torch.float64)
    gi32, _, _, _ = _oracle_grads(R.build_oracle50, "eval", imgs, spds, cmds, tgts, torch.float32)
    assert float((pc.detach().cpu().double() - oc).abs().max()) <= TOL_OUT
    _check_input_grad("ResNet-50 eval image.grad", x.grad, gi32, gi64)


# ---- no extra work when no input asks for a gradient --------------------------------------------
def test_profile_has_no_stem_dgrad_unless_an_input_requires_grad():
    imgs, spds, cmds, tgts = to_dev(*O.synthetic_batch(4, seed=8)[:4])
    m = make_model().train()
    pc, ps = m(imgs, spds, cmds)               # plan built outside the profiled window
    _loss(pc, ps, tgts, spds).backward()
    pl = m.engine().plan(4, imgs.size(2), imgs.size(3))
    pl.profile(True)
    try:
        pl.profile_reset()
        pc, ps = m(imgs, spds, cmds)
        _loss(pc, ps, tgts, spds).backward()
        torch.cuda.synchronize()
        rows = pl.profile_table()
        assert "conv_wgrad.stem" in rows and "conv_dgrad.stem" not in rows
        assert "heads_bwd.dspeed" not in rows
        pl.profile_reset()
        pc, ps = m(imgs.clone().requires_grad_(), spds, cmds)
        _loss(pc, ps, tgts, spds).backward()
        torch.cuda.synchronize()
        rows = pl.profile_table()
        assert rows["conv_dgrad.stem"]["calls"] == 1 and "heads_bwd.dspeed" not in rows
    finally:
        pl.profile(False)
