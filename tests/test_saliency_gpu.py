"""Saliency: the data-gradient-only backward (cilrs_net_backward_data), the reduction-free frozen
BatchNorm backward behind it (cilrs_bn_bwd_frozen / cilrs_bn_bwd_pool_frozen), the heat-map kernel
(cilrs_saliency_map) and Predictor.saliency on top of them.

Gates:
  data-only backward   image / speed gradients torch.equal to what the full backward gives for the
                       same graph; the gradient arena (filled with a sentinel) untouched
  frozen BN backward   exactly the torch fp32 expression  (z > 0 ? dz : 0) * (gamma * rstd)
  heat-map kernel      s and peak exactly torch's fp32 abs / mul / amax; heat within 1.2e-7 (one
                       rounding of a value <= 1); heat_u8 equal unless heat * 255 lies within 1e-4 of
                       a half
  Predictor.saliency   heat (and peak, relatively) against the float64 oracle: relative L2 error
                       <= max(4x the fp32 CPU oracle's own error, 5e-3) -- the input-gradient gate of
                       tests/test_input_grads_gpu.py
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cilrs_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5


def make_model(seed=0, dropout=0.0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=dropout)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda()


def make_model50():
    from cilrs_mi355 import CILRSResNet50
    m = CILRSResNet50(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    return m.cuda()


def to_dev(*ts):
    return [t.cuda() for t in ts]


def _loss(pc, ps, tgt, spd):
    return O.compute_loss(O.CONFIG_A, pc, tgt, ps, spd)[0]


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launched(rows):
    """Labels with launches since the last profile_reset (a reset keeps the labels it has seen)."""
    return {k: r for k, r in rows.items() if r["calls"] > 0}


def _full_then_data_only(m, imgs, spds, cmds, tgts, want_image=True):
    """One graph twice: loss.backward() with the parameters as they are (the full backward), then
    torch.autograd.grad on the inputs alone (the data-gradient-only backward) with the gradient
    arena full of a sentinel.  Returns the two pairs of gradients."""
    eng = m.engine()
    c, t = to_dev(cmds, tgts)
    x = imgs.cuda().requires_grad_(want_image)
    v = spds.cuda().requires_grad_()
    pc, ps = m(x, v, c)
    _loss(pc, ps, t, spds.cuda()).backward()
    full = (x.grad.clone() if want_image else None, v.grad.clone())
    torch.cuda.synchronize()
    eng.grads.fill_(SENTINEL)
    x2 = imgs.cuda().requires_grad_(want_image)
    v2 = spds.cuda().requires_grad_()
    pc, ps = m(x2, v2, c)
    got = torch.autograd.grad(_loss(pc, ps, t, spds.cuda()), (x2, v2) if want_image else (v2,))
    torch.cuda.synchronize()
    assert torch.equal(eng.grads, torch.full_like(eng.grads, SENTINEL))     # arena untouched
    assert eng._scratch_grads is None                                       # and no second arena
    return full, ((got[0], got[1]) if want_image else (None, got[0]))


# ---- 1 + 2. eval mode: bit-identity and the profile of the data-only pass -------------------------
@pytest.fixture(scope="module")
def eval_b4(golden_dir):
    g = np.load(os.path.join(golden_dir, "forward_eval_b4.npz"))
    imgs, spds, _, tgts = O.synthetic_batch(4, seed=int(g["seed"]))[:4]
    cmds = torch.from_numpy(g["command"])
    m = make_model().eval()
    eng = m.engine()
    bn_before, nbt_before = eng.bn.clone(), eng.nbt.clone()
    c, t = to_dev(cmds, tgts)
    # reference: trainable parameters, loss.backward()
    x = imgs.cuda().requires_grad_()
    v = spds.cuda().requires_grad_()
    pc, ps = m(x, v, c)
    _loss(pc, ps, t, spds.cuda()).backward()
    pl = eng.plan(4, imgs.size(2), imgs.size(3))
    # the same two passes again under the per-kernel profile
    rows = {}
    pl.profile(True)
    try:
        pl.profile_reset()
        xp = imgs.cuda().requires_grad_()
        pc, ps = m(xp, spds.cuda().requires_grad_(), c)
        _loss(pc, ps, t, spds.cuda()).backward()
        torch.cuda.synchronize()
        rows["full"] = _launched(pl.profile_table())
        full_profiled = xp.grad.clone()
    finally:
        pl.profile(False)
    # under test: every parameter frozen, torch.autograd.grad on the inputs
    m.requires_grad_(False)
    torch.cuda.synchronize()
    eng.grads.fill_(SENTINEL)
    x2 = imgs.cuda().requires_grad_()
    v2 = spds.cuda().requires_grad_()
    pc, ps = m(x2, v2, c)
    gx, gv = torch.autograd.grad(_loss(pc, ps, t, spds.cuda()), (x2, v2))
    torch.cuda.synchronize()
    arena_intact = torch.equal(eng.grads, torch.full_like(eng.grads, SENTINEL))
    pl.profile(True)
    try:
        pl.profile_reset()
        x3 = imgs.cuda().requires_grad_()
        pc, ps = m(x3, spds.cuda().requires_grad_(), c)
        (gx_profiled,) = torch.autograd.grad(_loss(pc, ps, t, spds.cuda()), (x3,))
        torch.cuda.synchronize()
        rows["data"] = _launched(pl.profile_table())
    finally:
        pl.profile(False)
    return dict(ref=(x.grad, v.grad), got=(gx, gv), arena_intact=arena_intact,
                scratch=eng._scratch_grads, rows=rows, profiled=(full_profiled, gx_profiled),
                bn_same=torch.equal(eng.bn, bn_before) and torch.equal(eng.nbt, nbt_before))


def test_eval_mode_data_only_backward_is_bit_identical(eval_b4):
    r = eval_b4
    assert torch.equal(r["got"][0], r["ref"][0])
    assert torch.equal(r["got"][1], r["ref"][1])
    assert torch.equal(r["profiled"][1], r["profiled"][0])      # serialised (profiled) launches too
    assert torch.equal(r["profiled"][1], r["ref"][0])
    assert r["arena_intact"]
    assert r["scratch"] is None
    assert r["bn_same"]


def test_eval_mode_data_only_backward_profile(eval_b4):
    full, data = eval_b4["rows"]["full"], eval_b4["rows"]["data"]
    assert any(k.startswith("conv_wgrad") for k in full)
    assert not [k for k in data if k.startswith("conv_wgrad")]
    assert data["heads_bwd"]["calls"] < full["heads_bwd"]["calls"]
    assert data["conv_dgrad.stem"]["calls"] == 1
    # the chain itself is the same: as many BatchNorm backwards and data gradients as the full pass
    for grp in ("layer1", "layer2", "layer3", "layer4", "stem"):
        assert data["bn_bwd." + grp]["calls"] == full["bn_bwd." + grp]["calls"]
        assert data["conv_dgrad." + grp]["calls"] == full["conv_dgrad." + grp]["calls"]


# ---- 3. train mode, the bf16 training plan, the ResNet-50 variant ---------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_mode_data_only_backward_is_bit_identical(golden_dir, precision):
    g = np.load(os.path.join(golden_dir, "forward_train_b8.npz"))
    imgs, spds, cmds, tgts = O.synthetic_batch(8, seed=int(g["seed"]))[:4]
    m = make_model().train()
    m.engine().train_precision = precision
    full, got = _full_then_data_only(m, imgs, spds, cmds, tgts)
    assert torch.isfinite(full[0]).all() and float(full[0].abs().max()) > 0
    assert torch.equal(got[0], full[0])
    assert torch.equal(got[1], full[1])


def test_resnet50_eval_data_only_backward_is_bit_identical():
    imgs, spds, cmds, tgts = O.synthetic_batch(2, seed=31, h=64, w=96)[:4]
    m = make_model50().eval()
    full, got = _full_then_data_only(m, imgs, spds, cmds, tgts)
    assert float(full[0].abs().max()) > 0
    assert torch.equal(got[0], full[0])
    assert torch.equal(got[1], full[1])


# ---- 4. the speed gradient alone ---------------------------------------------------------------------
def _speed_only_profile(m, imgs, spds, cmds, tgts):
    eng = m.engine()
    c, t = to_dev(cmds, tgts)
    pl = eng.plan(imgs.size(0), imgs.size(2), imgs.size(3))
    pl.profile(True)
    try:
        pl.profile_reset()
        v = spds.cuda().requires_grad_()
        pc, ps = m(imgs.cuda(), v, c)
        (gv,) = torch.autograd.grad(_loss(pc, ps, t, spds.cuda()), (v,))
        torch.cuda.synchronize()
        rows = _launched(pl.profile_table())
    finally:
        pl.profile(False)
    return gv, rows


def test_speed_gradient_alone_runs_the_heads_only():
    imgs, spds, cmds, tgts = O.synthetic_batch(4, seed=8)[:4]
    m = make_model().eval()
    full, got = _full_then_data_only(m, imgs, spds, cmds, tgts, want_image=False)
    assert float(full[1].abs().max()) > 0
    assert torch.equal(got[1], full[1])
    gv, rows = _speed_only_profile(m, imgs, spds, cmds, tgts)
    assert torch.equal(gv, full[1])
    assert "heads_bwd.dspeed" in rows
    assert not [k for k in rows if k.startswith(("conv_dgrad", "bn_bwd", "conv_wgrad"))]


def test_speed_gradient_alone_behind_a_fine_tuning_cut():
    imgs, spds, cmds, tgts = O.synthetic_batch(4, seed=8)[:4]
    m = make_model().train()
    m.freeze("layer2")
    full, got = _full_then_data_only(m, imgs, spds, cmds, tgts, want_image=False)
    assert float(full[1].abs().max()) > 0
    assert torch.equal(got[1], full[1])
    gv, rows = _speed_only_profile(m, imgs, spds, cmds, tgts)
    assert torch.equal(gv, full[1])
    assert not [k for k in rows if k.startswith(("conv_dgrad", "bn_bwd", "conv_wgrad"))]
    # an image gradient behind the cut is still refused
    with pytest.raises(RuntimeError, match="frozen"):
        m(imgs.cuda().requires_grad_(), spds.cuda(), cmds.cuda())


# ---- 5. the frozen BatchNorm backward, op level ------------------------------------------------------
@pytest.mark.parametrize("M,Cc", [(35, 64), (1100, 128), (312, 512), (42, 2048)])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_g_out", [False, True])
def test_bn_bwd_frozen_is_the_torch_expression(M, Cc, relu, with_g_out):
    L = _lib()
    g = torch.Generator().manual_seed(M * 7 + Cc + relu)
    dz = torch.randn(M, Cc, generator=g)
    z = F.relu(torch.randn(M, Cc, generator=g))                 # many exact zeros
    gamma = torch.randn(Cc, generator=g)
    stats = torch.randn(4 * Cc, generator=g)
    stats[Cc:2 * Cc] = torch.rand(Cc, generator=g) + 0.5        # rstd
    gg = torch.where(z > 0, dz, torch.zeros_like(dz)) if relu else dz
    want = gg * (gamma * stats[Cc:2 * Cc])
    dzd, zd, gd, sd = to_dev(dz, z, gamma, stats)
    outs = []
    for _ in range(2):
        dy = torch.full((M, Cc), float("nan"), device="cuda")
        g_out = torch.full((M, Cc), float("nan"), device="cuda") if with_g_out else None
        L.check(L.lib().cilrs_bn_bwd_frozen(L.ptr(dzd), L.ptr(zd) if relu else None, M, Cc,
                                            L.ptr(gd), L.ptr(sd), relu, L.ptr(dy), L.ptr(g_out),
                                            stream()))
        torch.cuda.synchronize()
        outs.append((dy, g_out))
    assert not torch.isnan(outs[0][0]).any()                     # every element written
    assert torch.equal(outs[0][0].cpu(), want)
    assert torch.equal(outs[0][0], outs[1][0])
    if with_g_out:
        assert torch.equal(outs[0][1].cpu(), gg)
        assert torch.equal(outs[0][1], outs[1][1])


def test_bn_bwd_frozen_refuses_a_channel_count_it_cannot_serve():
    """3072 channels pass the BatchNorm family's common check, but C/4 = 768 does not divide the
    kernel's 1,024-thread stride: refused, nothing launched."""
    L = _lib()
    M, Cc = 8, 3072
    dz, gamma, stats = torch.ones(M, Cc, device="cuda"), torch.ones(Cc, device="cuda"), \
        torch.ones(4 * Cc, device="cuda")
    dy = torch.full((M, Cc), float("nan"), device="cuda")
    with pytest.raises(RuntimeError, match="unsupported channel count"):
        L.check(L.lib().cilrs_bn_bwd_frozen(L.ptr(dz), None, M, Cc, L.ptr(gamma), L.ptr(stats), 0,
                                            L.ptr(dy), None, stream()))
    torch.cuda.synchronize()
    assert torch.isnan(dy).all()


@pytest.mark.parametrize("N,H,W", [(2, 44, 100), (1, 19, 26)])
def test_bn_bwd_pool_frozen_is_the_torch_expression(N, H, W):
    """maxpool3x3/s2/p1(relu(y * scale + shift)) backwards.  The inputs are small dyadic numbers:
    y * scale + shift and the (up to four) gradients that meet in one pixel sum exactly, so the
    torch expression has one value whatever the order of the additions."""
    L = _lib()
    Cc = 64
    g = torch.Generator().manual_seed(H * W)
    y = torch.randint(-32, 33, (N, H, W, Cc), generator=g).float() / 8
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (Cc,), generator=g)]
    shift = torch.randint(-8, 9, (Cc,), generator=g).float() / 8
    gamma = torch.randn(Cc, generator=g)
    rstd = torch.rand(Cc, generator=g) + 0.5
    stats = torch.cat([torch.randn(Cc, generator=g), rstd, scale, shift])
    z = y * scale + shift
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dpool = torch.randint(-16, 17, (N, Ho, Wo, Cc), generator=g).float() / 4
    a = F.relu(z).cuda().contiguous()
    pooled = torch.empty(N, Ho, Wo, Cc, device="cuda")
    am = torch.empty(N, Ho, Wo, Cc, dtype=torch.uint8, device="cuda")
    L.check(L.lib().cilrs_maxpool_fwd(L.ptr(a), L.ptr(pooled), L.ptr(am), N, H, W, Cc, stream()))
    torch.cuda.synchronize()
    # torch: scatter each window's gradient to its argmax tap, mask by z > 0, scale
    k = am.cpu().long()
    n_i, oh, ow, c_i = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Wo),
                                      torch.arange(Cc), indexing="ij")
    ih, iw = 2 * oh - 1 + k // 3, 2 * ow - 1 + k % 3
    assert int(ih.min()) >= 0 and int(ih.max()) < H and int(iw.min()) >= 0 and int(iw.max()) < W
    scat = torch.zeros(N, H, W, Cc)
    scat.index_put_((n_i.flatten(), ih.flatten(), iw.flatten(), c_i.flatten()), dpool.flatten(),
                    accumulate=True)
    want = torch.where(z > 0, scat, torch.zeros_like(scat)) * (gamma * rstd)
    yd, dpd, gd, sd = to_dev(y, dpool, gamma, stats)
    outs = []
    for _ in range(2):
        dy = torch.full((N, H, W, Cc), float("nan"), device="cuda")
        L.check(L.lib().cilrs_bn_bwd_pool_frozen(L.ptr(dpd), L.ptr(am), L.ptr(yd), N, H, W, Cc,
                                                 L.ptr(gd), L.ptr(sd), L.ptr(dy), stream()))
        torch.cuda.synchronize()
        outs.append(dy)
    assert not torch.isnan(outs[0]).any()
    assert float(want.abs().max()) > 0
    assert torch.equal(outs[0].cpu(), want)
    assert torch.equal(outs[0], outs[1])


# ---- 6. the heat-map kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 88, 200), (1, 37, 51)])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("scaled", [False, True, "pinned"])
def test_saliency_map_kernel(B, H, W, channels_last, scaled):
    """scaled = "pinned": per-level scales on channels 0 and 2, scale 1 on channel 1, whose values
    are small apart from one planted -4 -- the peak is 4 exactly, so heat * 4 is s itself and every
    scaled product is held element for element."""
    L = _lib()
    g = torch.Generator().manual_seed(B * 100 + H + (7 if scaled else 0))
    d = torch.randn(B, 3, H, W, generator=g).clamp_(-3.5, 3.5)
    d[0, 1, H // 2, W // 3] = -4.0              # unscaled: peak[0] = 4 exactly, so heat * 4 == s
    if B > 1:
        d[1] = 0.0                              # an all-zero frame
    scale3 = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)] if scaled else None
    if scaled == "pinned":
        scale3[1] = 1.0
        d[:, 1] *= 0.015625                     # comparable to the other channels' scaled values
        d[0, 1, H // 2, W // 3] = -4.0
    sc = torch.tensor(scale3 if scaled else [1.0, 1.0, 1.0], dtype=torch.float32)
    s_ref = (d.abs() * sc.view(1, 3, 1, 1)).amax(1)
    peak_ref = s_ref.amax((1, 2))
    heat_ref = torch.where(peak_ref.view(B, 1, 1) > 0, s_ref / peak_ref.view(B, 1, 1).clamp_min(1e-38),
                           torch.zeros_like(s_ref))
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    dd = d.cuda().contiguous(memory_format=fmt)
    cs = (C.c_float * 3)(*scale3) if scaled else None
    outs = []
    for _ in range(2):
        heat = torch.full((B, H, W), float("nan"), device="cuda")
        heat_u8 = torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda")
        peak = torch.full((B,), float("nan"), device="cuda")
        L.check(L.lib().cilrs_saliency_map(L.ptr(dd), *dd.stride(), B, H, W, cs, L.ptr(heat),
                                           L.ptr(heat_u8), L.ptr(peak), stream()))
        torch.cuda.synchronize()
        outs.append((heat, heat_u8, peak))
    heat, heat_u8, peak = (t.cpu() for t in outs[0])
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert not torch.isnan(heat).any() and not torch.isnan(peak).any()
    assert torch.equal(peak, peak_ref)
    if scaled is not True:
        assert float(peak[0]) == 4.0
        assert torch.equal(heat[0] * 4.0, s_ref[0])            # s itself, exactly
    assert float((heat - heat_ref).abs().max()) <= 1.2e-7
    assert float(heat.max()) == 1.0
    x255 = heat_ref.double() * 255.0
    decided = (x255 - torch.floor(x255) - 0.5).abs() > 1e-4
    want_u8 = torch.floor(x255 + 0.5).to(torch.uint8)
    assert torch.equal(heat_u8[decided], want_u8[decided])
    assert int((heat_u8.int() - want_u8.int()).abs().max()) <= 1
    if B > 1:
        assert float(peak[1]) == 0.0 and float(heat[1].abs().max()) == 0.0
        assert int(heat_u8[1].max()) == 0
    # heat_u8 and peak are optional
    heat2 = torch.full((B, H, W), float("nan"), device="cuda")
    L.check(L.lib().cilrs_saliency_map(L.ptr(dd), *dd.stride(), B, H, W, cs, L.ptr(heat2), None,
                                       None, stream()))
    torch.cuda.synchronize()
    assert torch.equal(heat2, outs[0][0])


# ---- 7. Predictor.saliency against the oracle -----------------------------------------------------------
OUTPUT_W = {"steer": (1.0, 0.0, 0.0, 0.0), "speed": (0.0, 0.0, 0.0, 1.0)}
IMG_STD = (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def oracles():
    return {torch.float64: O.build_oracle(0).double().eval(), torch.float32: O.build_oracle(0).eval()}


def _oracle_saliency(orc, x, speeds_kmh, commands, weights, dtype):
    """The definition: d (w . (controls, pred_speed)) / d image of the eval-mode oracle, max over
    the colour channels of its magnitude per 8-bit pixel level, normalised per frame."""
    x = x.detach().clone().to(dtype).requires_grad_()
    spd = torch.tensor([min(s / O.SPEED_NORM, 1.0) for s in speeds_kmh], dtype=dtype)
    pc, ps = orc(x, spd, torch.tensor(commands, dtype=torch.long))
    w = torch.tensor(weights, dtype=dtype)
    ((pc * w[:3]).sum() + (ps * w[3]).sum()).backward()
    scale = torch.tensor([1.0 / (255.0 * s) for s in IMG_STD], dtype=dtype).view(1, 3, 1, 1)
    s = (x.grad.abs() * scale).amax(1)
    peak = s.amax((1, 2))
    return (s / peak.view(-1, 1, 1)).double(), peak.double(), pc.detach(), ps.detach()


def _rel(a, ref):
    return float((a.double() - ref).norm()) / max(float(ref.norm()), 1e-30)


def _check_saliency(tag, got, x, speeds, cmds, output, oracles, pb):
    out, heat, peak = got
    B = x.size(0)
    assert out.shape == (B, 4) and out.dtype == np.float32
    assert heat.shape == (B, 88, 200) and heat.dtype == np.float32 and peak.shape == (B,)
    h64, p64, _, _ = _oracle_saliency(oracles[torch.float64], x, speeds, cmds, OUTPUT_W[output],
                                      torch.float64)
    h32, p32, _, _ = _oracle_saliency(oracles[torch.float32], x, speeds, cmds, OUTPUT_W[output],
                                      torch.float32)
    e_gpu, e_cpu = _rel(torch.from_numpy(heat), h64), _rel(h32, h64)
    pe_gpu = float(((torch.from_numpy(peak).double() - p64).abs() / p64).max())
    pe_cpu = float(((p32 - p64).abs() / p64).max())
    print(f"{tag}: heat relative L2 vs float64 {e_gpu:.3e} (fp32 CPU oracle {e_cpu:.3e}); peak "
          f"relative error {pe_gpu:.3e} (CPU {pe_cpu:.3e})")
    assert (peak > 0).all() and float(heat.max()) == 1.0 and float(heat.min()) >= 0.0
    assert e_gpu <= max(4.0 * e_cpu, 5e-3), (tag, e_gpu, e_cpu)
    assert pe_gpu <= max(4.0 * pe_cpu, 5e-3), (tag, pe_gpu, pe_cpu)
    assert np.abs(out[:, :3] - pb[:, :3]).max() <= 1e-4
    assert np.abs(out[:, 3] - pb[:, 3]).max() <= 90e-4


@pytest.mark.parametrize("B", [1, 2])
def test_predictor_saliency_vs_oracle(B, oracles):
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(B, seed=40 + B)[4]
    speeds, cmds = [12.0, 55.0][:B], [2, 0][:B]
    x = torch.cat([O.preprocess_frame(f) for f in u8])
    m = make_model()
    pr = Predictor(m, batch=B)                  # B = 1: the default, persistent predictor
    before = pr.predict_batch(u8, speeds, cmds)
    for output in ("steer", "speed"):
        got = pr.saliency(u8, speeds, cmds, output=output)
        _check_saliency(f"B={B} {output}", got, x, speeds, cmds, output, oracles, before)
        # four weights name the same thing, and the call is reproducible
        again = pr.saliency(u8, speeds, cmds, output=OUTPUT_W[output])
        for a, b in zip(got, again):
            assert np.array_equal(a, b)
    after = pr.predict_batch(u8, speeds, cmds)
    assert np.array_equal(before, after)        # the predictor's own state is not disturbed


def test_predictor_saliency_camera_frame(oracles):
    from cilrs_mi355.predict import Predictor
    cam = np.floor(O._hash_u01(5, 9, 600 * 800 * 4) * 256).astype(np.uint8).reshape(1, 600, 800, 4)
    pr = Predictor(make_model())
    small = O.resize_bilinear_u8(np.ascontiguousarray(cam[0, :, :, :3]))[None]
    pb = pr.predict_batch(small, [30.0], [1])
    got = pr.saliency(cam, [30.0], [1])
    _check_saliency("camera steer", got, O.preprocess_camera(cam[0]), [30.0], [1], "steer", oracles, pb)
    via_u8 = pr.saliency(small, [30.0], [1])    # the device resize is the oracle's, pixel for pixel
    for a, b in zip(got, via_u8):
        assert np.array_equal(a, b)


def test_predictor_saliency_misuse_raises_before_any_launch():
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(1, seed=3)[4]
    m = make_model()
    pr = Predictor(m)
    eng = m.engine()
    params, epoch, plans = eng.params.clone(), eng.weights_epoch, len(eng.plans)
    with pytest.raises(ValueError):
        pr.saliency(u8, [10.0], [1], output="steering")
    with pytest.raises(ValueError):
        pr.saliency(u8, [10.0], [1], output=[1.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match="out of range"):
        pr.saliency(u8, [10.0], [4])
    with pytest.raises(RuntimeError):
        pr.saliency(u8[0], [10.0], [1])                          # not a batch of frames
    with pytest.raises(RuntimeError):
        pr.saliency(u8.astype(np.float32), [10.0], [1])
    torch.cuda.synchronize()
    assert torch.equal(eng.params, params) and eng.weights_epoch == epoch
    assert len(eng.plans) == plans and getattr(pr, "_sal", None) is None      # nothing was set up
