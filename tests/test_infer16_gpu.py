"""The 16-bit inference trunk (cilrs_net_forward_u8_f16 / _bf16), kernel by kernel against its CPU
definition oracle/infer16_emulation.py, then the whole network layer by layer and bit for bit.

Every stored 16-bit result is compared with the float64 value BEFORE the final rounding, computed
from the SAME stored 16-bit operands the kernel got (so the only freedom is the order of an fp32
sum).  Two assertions per tensor, no element left out:

  bound   |got - ref| <= h(ref) + tiny + 1e-6 * max|ref|,  h(ref) = 2^(floor(log2|ref|) - p) = half
          the 16-bit spacing in ref's binade (p = 11 fp16, 8 bf16; tiny = 2^-25 for fp16, half its
          subnormal spacing): a correct rounding of something at fp32-summation distance from ref.
          A truncation (error up to a full spacing) fails it.
  share   the share of elements whose stored value differs from round_T(ref) must not exceed
          max(8 x the share of torch's fp32 CPU realisation of the same step, 32 / n): that share is
          proportional to the accumulation error, two fp32 summation orders differ in it by a small
          factor; a second rounding or another rounding mode puts it above 0.1.

Largest flip shares observed on an MI355X (op tests, folds and walks of this file together, 407
tensors per type): fp16 1.79e-3 (conv (2,6,7,2048,512,1,1,0), relu off; torch's fp32 realisation
2.44e-3 there), bf16 2.79e-4 (conv (1,3,7,512,512,3,1,1), relu off; torch 9.3e-5).  No share came
closer to its cap than 0.31 x, no element closer to the bound than the bound itself (worst 1.000).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cilrs_oracle as O
import infer16_emulation as E
from test_ops_gpu import CONV_CASES

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
# name -> (torch type, bf16 flag of the C-ABI, `half` of Engine.run_forward_u8, tiny, fold code)
TYPES = {"fp16": (torch.float16, 0, True, 2.0 ** -25, 1),
         "bf16": (torch.bfloat16, 1, "bf16", 0.0, 2)}
_SHARES = {"fp16": [], "bf16": []}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the kernels, CPU tensors in and out (16-bit tensors NHWC / OHWI as the engine keeps them) ----
def hip_conv(x, w, bias, res, k, s, p, relu, bf16, tile=0):
    L = _lib()
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xd, wd, bd = x.contiguous().cuda(), w.contiguous().cuda(), bias.contiguous().cuda()
    rd = None if res is None else res.contiguous().cuda()
    y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=x.dtype, device="cuda")
    L.check(L.lib().cilrs_conv2d_infer_16(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(rd), L.ptr(y), N, H,
                                          W, Cin, Cout, k, s, p, relu, bf16, tile, _stream()))
    torch.cuda.synchronize()
    return y.cpu()


def hip_stem_fold(w_ohwi, stats, T, bf16):
    L = _lib()
    wd, sd = w_ohwi.contiguous().cuda(), stats.contiguous().cuda()
    w16 = torch.full((64, 7, 8, 4), float("nan"), dtype=T, device="cuda")
    bias = torch.full((64,), float("nan"), device="cuda")
    L.check(L.lib().cilrs_stem_fold_16(L.ptr(wd), L.ptr(sd), L.ptr(w16), L.ptr(bias), bf16, _stream()))
    torch.cuda.synchronize()
    return w16.cpu(), bias.cpu()


def hip_stem(x4, w16, bias, bf16):
    L = _lib()
    N, H, W, _ = x4.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd, wd, bd = x4.contiguous().cuda(), w16.contiguous().cuda(), bias.contiguous().cuda()
    z = torch.full((N, Ho, Wo, 64), float("nan"), dtype=w16.dtype, device="cuda")
    L.check(L.lib().cilrs_stem_infer_16(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(z), N, H, W, bf16,
                                        _stream()))
    torch.cuda.synchronize()
    return z.cpu()


def hip_maxpool(x, bf16):
    L = _lib()
    N, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = x.contiguous().cuda()
    out = torch.full((N, Ho, Wo, Cc), float("nan"), dtype=x.dtype, device="cuda")
    L.check(L.lib().cilrs_maxpool_infer_16(L.ptr(xd), L.ptr(out), N, H, W, Cc, bf16, _stream()))
    torch.cuda.synchronize()
    return out.cpu()


def hip_avgpool(x, out, bf16):
    """x [N][HW][C] 16-bit, out [N][ld] fp32 (pre-filled by the caller); returns the filled copy."""
    L = _lib()
    N, HW, Cc = x.shape
    xd, od = x.contiguous().cuda(), out.contiguous().cuda()
    L.check(L.lib().cilrs_avgpool_infer_16(L.ptr(xd), L.ptr(od), N, HW, Cc, out.shape[1], bf16,
                                           _stream()))
    torch.cuda.synchronize()
    return od.cpu()


def nchw(t):                     # stored NHWC tensor -> NCHW fp32 values (exact)
    return t.float().permute(0, 3, 1, 2).contiguous()


def oihw(w):                     # stored OHWI weights -> OIHW fp32 values (exact)
    return w.float().permute(0, 3, 1, 2).contiguous()


# ---- the two assertions ----------------------------------------------------------------------------
def check_stored(got, ref, cpu32, tname, what, floor=None):
    """got: what the kernel stored (values, any float dtype, ref's layout); ref: float64 before the
    rounding; cpu32: the fp32 CPU realisation's stored values.  Returns the kernel's flip share."""
    T, tiny = TYPES[tname][0], TYPES[tname][3]
    g = got.double()
    assert g.shape == ref.shape and ref.dtype == torch.float64
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    fl = 1e-6 * float(ref.abs().max()) if floor is None else floor
    err = (g - ref).abs()
    bound = E.half_spacing(ref, T) + tiny + fl
    want = E.round_to(ref, T)
    n = ref.numel()
    share = float((g != want).sum()) / n
    share_cpu = float((cpu32.double() != want).sum()) / n
    cap = max(8.0 * share_cpu, 32.0 / n)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"INFER16 {tname} {what}: n={n} worst err/bound {worst:.3f}  flip share hip {share:.3e} "
          f"cpu32 {share_cpu:.3e} cap {cap:.3e}")
    _SHARES[tname].append(share)
    nbad = int((err > bound).sum())
    wrong = []                                   # both assertions, reported together
    if nbad:
        wrong.append(f"{nbad}/{n} elements beyond half a spacing (worst {worst:.3f} x bound)")
    if share > cap:
        wrong.append(f"flip share {share:.3e} > cap {cap:.3e} (cpu32 {share_cpu:.3e})")
    assert not wrong, f"{what}: " + "; ".join(wrong)
    return share


# ---- convolution ---------------------------------------------------------------------------------
BOTTLENECK_CASES = [
    (2, 11, 13, 256, 1024, 1, 1, 0), (2, 6, 7, 2048, 512, 1, 1, 0), (2, 22, 50, 64, 256, 1, 1, 0),
    (2, 11, 13, 512, 2048, 1, 2, 0), (2, 22, 50, 128, 128, 3, 2, 1),
]
RAGGED_CASES = [                                  # M = 63, 64, 65, 127, 128, 129; 6 (< one tile)
    (1, 9, 7, 64, 128, 3, 1, 1), (1, 8, 8, 64, 128, 3, 1, 1), (1, 5, 13, 64, 128, 3, 1, 1),
    (1, 1, 127, 64, 128, 3, 1, 1), (1, 8, 16, 64, 128, 3, 1, 1), (1, 3, 43, 64, 128, 3, 1, 1),
    (1, 2, 3, 64, 128, 3, 1, 1),
    (64, 22, 50, 64, 64, 3, 1, 1),                # serving size
]
ALL_CONV_CASES = list(CONV_CASES) + BOTTLENECK_CASES + RAGGED_CASES


def _conv_operands(case, T, seed):
    N, H, W, Cin, Cout, k, s, p = case
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = F.relu(torch.randn(N, H, W, Cin, generator=g)).to(T)
    w = (torch.randn(Cout, k, k, Cin, generator=g) / (k * k * Cin) ** 0.5).to(T)
    bias = 0.2 * torch.randn(Cout, generator=g)
    res = F.relu(torch.randn(N, Ho, Wo, Cout, generator=g)).to(T)
    return x, w, bias, res


def _run_conv_case(case, tname, x, w, bias, res, variants):
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    N, H, W, Cin, Cout, k, s, p = case
    xs, ws_ = nchw(x), oihw(w)
    acc64 = F.conv2d(xs.double(), ws_.double(), None, s, p)           # once per case
    acc32 = F.conv2d(xs, ws_, None, s, p)
    r64, r32 = nchw(res).double(), nchw(res)
    b64, b32 = bias.double().view(1, -1, 1, 1), bias.view(1, -1, 1, 1)
    tiles = (0, 128) if Cout % 128 == 0 else (0,)
    for relu, with_res in variants:
        ref = acc64 + b64
        c32 = acc32 + b32
        if with_res:
            ref, c32 = ref + r64, c32 + r32
        if relu:
            ref, c32 = F.relu(ref), F.relu(c32)
        c32 = E.round_to(c32, T)
        for tile in tiles:
            y = hip_conv(x, w, bias, res if with_res else None, k, s, p, relu, bf16, tile)
            check_stored(nchw(y), ref, c32, tname,
                         f"conv {case} relu={relu} residual={int(with_res)} tile={tile or 64}")


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ALL_CONV_CASES)
def test_infer16_conv_is_one_rounding_of_the_float64_value(case, tname):
    """conv_f16_kernel's inference epilogue, 64x64 tile and (Cout % 128 == 0) 128x128 tile:
    round_T(relu?((acc + bias) + residual)) for (relu, residual) in (1, no), (1, yes), (0, no)."""
    T = TYPES[tname][0]
    x, w, bias, res = _conv_operands(case, T, 31)
    _run_conv_case(case, tname, x, w, bias, res, [(1, False), (1, True), (0, False)])


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
def test_infer16_conv_rounds_once_after_the_residual(tname):
    """bias 1.0, accumulators and residuals uniform in [0, half a spacing at 1.0): rounding
    acc + bias BEFORE the residual is added gives 1.0 everywhere, the single rounding gives the
    next value up wherever acc + residual exceeds half a spacing -- about half of the elements."""
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    p = 11 if tname == "fp16" else 8
    N, H, W, Cin, Cout = 2, 9, 13, 64, 128
    g = torch.Generator().manual_seed(77)
    hot = torch.randint(0, Cin, (N, H, W, 1), generator=g)
    x = torch.zeros(N, H, W, Cin).scatter_(3, hot, torch.rand(N, H, W, 1, generator=g)).to(T)
    w = ((0.5 + 0.5 * torch.rand(Cout, 1, 1, Cin, generator=g)) * 2.0 ** -p).to(T)
    bias = torch.ones(Cout)
    res = (torch.rand(N, H, W, Cout, generator=g) * 2.0 ** -p).to(T)
    acc = F.conv2d(nchw(x).double(), oihw(w).double())
    once = E.round_to(acc + 1.0 + nchw(res).double(), T)
    twice = E.round_to(E.round_to(acc + 1.0, T) + nchw(res).double(), T)
    differ = float((once != twice).double().mean())
    print(f"INFER16 {tname} rounding-point case: the two formulas differ on {differ:.3f} of the elements")
    assert differ >= 0.1
    _run_conv_case((N, H, W, Cin, Cout, 1, 1, 0), tname, x, w, bias, res, [(1, True)])


# ---- stem, pools ---------------------------------------------------------------------------------
def _bn_params(C_, g):
    gamma = (0.5 + torch.rand(C_, generator=g)) * torch.where(torch.rand(C_, generator=g) < 0.4, -1.0, 1.0)
    gamma[5] = 0.0
    beta = 0.3 * torch.randn(C_, generator=g)
    mean = 0.3 * torch.randn(C_, generator=g)
    var = 10.0 ** (torch.rand(C_, generator=g) * 5.0 - 3.0)
    var[0], var[1] = 1e-3, 1e2
    return gamma, beta, mean, var


def _check_stem(x4, w16, bias, z, tname):
    """stem_f16_kernel's stored output against the float64 convolution of the kernel's OWN folded
    weights and the image rounded to T."""
    T = TYPES[tname][0]
    img = x4[..., :3].permute(0, 3, 1, 2).contiguous()
    wf = w16[:, :, :7, :3].float().permute(0, 3, 1, 2).contiguous()
    ref = E.stem_pre(img, wf, bias, T, torch.float64)
    c32 = E.round_to(E.stem_pre(img, wf, bias, T, torch.float32), T)
    return check_stored(nchw(z), ref, c32, tname, f"stem {tuple(x4.shape[:3])}")


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("N,H,W", [(5, 88, 200), (2, 176, 400), (1, 88, 200), (3, 9, 253),
                                   (2, 61, 445), (2, 30, 70)])
def test_infer16_stem_and_its_fold(N, H, W, tname):
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    g = torch.Generator().manual_seed(41)
    w = torch.randn(64, 7, 7, 3, generator=g) / 147 ** 0.5
    gamma, beta, mean, var = _bn_params(64, g)
    scale, shift = E.fold_scale_shift(gamma, beta, mean, var)
    stats = torch.cat([mean, 1.0 / torch.sqrt(var + E.BN_EPS), scale, shift])
    w16, bias = hip_stem_fold(w, stats, T, bf16)
    assert torch.equal(bias, shift)
    assert (w16[:, :, 7, :].float() == 0).all() and (w16[:, :, :, 3].float() == 0).all()   # pad taps
    got = w16[:, :, :7, :3].float()
    ref = w.double() * scale.double().view(-1, 1, 1, 1)
    c32 = E.round_to(w * scale.view(-1, 1, 1, 1), T)
    check_stored(got, ref, c32, tname, "stem fold", floor=1e-6 * ref.abs())
    assert (got[5] == 0).all()                                        # the gamma == 0 channel
    x4 = torch.randn(N, H, W, 4, generator=g)
    x4[..., 3] = 3.0                     # the pad channel: inert only if its taps' weights are zero
    z = hip_stem(x4, w16, bias, bf16)
    _check_stem(x4, w16, bias, z, tname)


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("N,H,W", [(1, 7, 9), (3, 8, 8), (2, 44, 100)])
def test_infer16_maxpool_is_exact(N, H, W, tname):
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    x = torch.randn(N, H, W, 64, generator=torch.Generator().manual_seed(43)).to(T)
    got = hip_maxpool(x, bf16)
    want = E.maxpool(nchw(x)).permute(0, 2, 3, 1)
    assert got.shape == want.shape and torch.equal(got.float(), want)


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("HW", [21, 66])
@pytest.mark.parametrize("Cc", [512, 2048])
def test_infer16_avgpool_into_a_pitched_matrix(HW, Cc, tname):
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    N, ld = 3, Cc + 128
    x = F.relu(torch.randn(N, HW, Cc, generator=torch.Generator().manual_seed(47))).to(T)
    out = torch.full((N, ld), 7.5)
    out[:, :Cc] = float("nan")
    got = hip_avgpool(x, out, bf16)
    ref = x.double().sum(1) / HW
    assert torch.isfinite(got).all()
    assert (got[:, Cc:] == 7.5).all()                                  # beyond C: untouched
    err = float((got[:, :Cc].double() - ref).abs().max())
    print(f"INFER16 {tname} avgpool HW={HW} C={Cc}: max err {err:.3e} (max|ref| {float(ref.max()):.3f})")
    assert err <= 1e-6 * float(ref.abs().max())


# ---- a plan: the fold, the walk, bit equality ----------------------------------------------------
def _models(net, seed=0):
    """(engine-backed module on the GPU, CPU oracle), both with the perturbed-statistics weights."""
    if net == "resnet34":
        from cilrs_mi355 import CILRS
        m, orc = CILRS(4, 0.0), O.build_oracle(0)
    else:
        import resnet50_oracle as R
        from cilrs_mi355 import CILRSResNet50
        m, orc = CILRSResNet50(4, 0.0), R.build_oracle50(0)
    sd = E.perturbed_state_dict(O.portable_state_dict(orc.state_dict(), seed), seed)
    orc.load_state_dict(sd, strict=True)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), orc.eval()


def _conv_numbers(orc):
    """id(conv module) -> the engine's convolution number (parameter order: 0 the stem, then every
    block's conv1, conv2[, conv3][, downsample])."""
    convs = [m for _n, m in orc.visual_encoder.named_modules() if isinstance(m, torch.nn.Conv2d)]
    order = [n for n, p in orc.visual_encoder.named_parameters() if p.dim() == 4]
    mods = dict(orc.visual_encoder.named_modules())
    assert len(convs) == len(order)
    return {id(mods[n[:-len(".weight")]]): i for i, n in enumerate(order)}


class _PlanView:
    """What a plan's 16-bit forward read and wrote, through the accessors."""

    def __init__(self, pl, tname):
        self.pl, self.T, self.code = pl, TYPES[tname][0], TYPES[tname][4]
        self.L = _lib()

    def folded(self, ci):
        """(w16 in the engine's layout, flat; bias fp32), CPU copies."""
        lib = self.L.lib()
        wo, bo, wn, ch, half = self.L.sz(), self.L.sz(), self.L.sz(), self.L.i32(), self.L.i32()
        self.L.check(lib.cilrs_net_infer16_conv_info(self.pl.handle, ci, C.byref(wo), C.byref(bo),
                                                     C.byref(wn), C.byref(ch), C.byref(half)))
        assert half.value == self.code, "the plan's arenas do not hold this type's fold"
        ws = self.pl.workspace
        w16 = ws[wo.value:wo.value + 2 * wn.value].view(self.T).cpu()
        bias = ws[bo.value:bo.value + 4 * ch.value].view(torch.float32).cpu()
        return w16, bias

    def io(self):
        """(x4 [B][H][W][4] fp32, combined[:, :feat] fp32), CPU copies."""
        lib = self.L.lib()
        xo, xn, co, ld, feat = self.L.sz(), self.L.sz(), self.L.sz(), self.L.i32(), self.L.i32()
        self.L.check(lib.cilrs_net_infer16_io_info(self.pl.handle, C.byref(xo), C.byref(xn),
                                                   C.byref(co), C.byref(ld), C.byref(feat)))
        ws, pl = self.pl.workspace, self.pl
        x4 = ws[xo.value:xo.value + 4 * xn.value].view(torch.float32).cpu().view(pl.batch, pl.h, pl.w, 4)
        comb = ws[co.value:co.value + 4 * pl.batch * ld.value].view(torch.float32).cpu()
        return x4, comb.view(pl.batch, ld.value)[:, :feat.value].contiguous()


def _forward16(net, tname, B, H, W, seed=123):
    m, orc = _models(net)
    eng = m.engine()
    img, spd, cmd, _, u8 = O.synthetic_batch(B, seed=seed, h=H, w=W)
    c, s = eng.run_forward_u8(torch.from_numpy(u8).cuda(), spd.cuda(), cmd.cuda(),
                              half=TYPES[tname][2])
    torch.cuda.synchronize()
    return m, orc, eng, (img, spd, cmd), (c.cpu(), s.cpu()), _PlanView(eng.last_plan, tname)


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("net", ["resnet34", "resnet50"])
def test_infer16_fold_of_a_plan(net, tname):
    """fold_bn_f16_kernel / fold_stem_kernel through a plan's table: every convolution's folded
    weights against round_T(float64(w) * gamma / sqrt(var + eps)), biases within 1e-6 of the
    magnitude of their two terms, on statistics that differ from layer to layer."""
    T = TYPES[tname][0]
    m, orc, eng, _, _, view = _forward16(net, tname, 2, 88, 200)
    ve = orc.visual_encoder
    pairs = [(ve[0], ve[1])]
    for blk in E.trunk_blocks(orc):
        main, down = E.block_convs(blk)
        pairs += main + ([down] if down else [])
    numbers = _conv_numbers(orc)
    assert sorted(numbers[id(c)] for c, _ in pairs) == list(range(len(pairs)))
    assert len(pairs) == (36 if net == "resnet34" else 53)
    for conv, bn in pairs:
        ci = numbers[id(conv)]
        w16, bias = view.folded(ci)
        w = conv.weight.detach()
        if ci == 0:
            w16 = w16.view(64, 7, 8, 4)
            assert (w16[:, :, 7, :].float() == 0).all() and (w16[:, :, :, 3].float() == 0).all()
            got = w16[:, :, :7, :3].float().permute(0, 3, 1, 2)
        else:
            got = w16.view(w.shape[0], w.shape[2], w.shape[3], w.shape[1]).float().permute(0, 3, 1, 2)
        ref = E.fold_conv_bn_ref64(w, bn.weight.detach(), bn.running_var)
        c32, shift = E.fold_conv_bn(w, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                    bn.running_var, T)
        check_stored(got, ref, c32, tname, f"{net} fold conv {ci}", floor=1e-6 * ref.abs())
        scale64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + E.BN_EPS)
        b64 = bn.bias.detach().double() - bn.running_mean.double() * scale64
        mag = bn.bias.detach().double().abs() + (bn.running_mean.double() * scale64).abs()
        assert ((bias.double() - b64).abs() <= 1e-6 * mag).all(), f"{net} bias of conv {ci}"


def _walk(orc, x4, folded, tname):
    """Drive the op-level entries in the order of the ORACLE's module structure; every step gets the
    previous step's HIP output and is checked against the emulation's single step on that input.
    folded(conv module) -> (w16 in the engine's layout, bias).  Returns the pooled features."""
    T, bf16 = TYPES[tname][0], TYPES[tname][1]
    ve = orc.visual_encoder
    w16, bias = folded(ve[0])
    w16 = w16.view(64, 7, 8, 4)
    z = hip_stem(x4, w16, bias, bf16)
    _check_stem(x4, w16, bias, z, tname)
    x = hip_maxpool(z, bf16)
    assert torch.equal(nchw(x), E.maxpool(nchw(z)))
    nconv = 0

    def step(conv, xin, residual, relu, what):
        nonlocal nconv
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        wv, b = folded(conv)
        wv = wv.view(conv.out_channels, k, k, conv.in_channels)
        y = hip_conv(xin, wv, b, residual, k, s, p, relu, bf16)
        r = None if residual is None else nchw(residual)
        ref = E.conv_pre(nchw(xin), oihw(wv), b, r, bool(relu), s, p, torch.float64)
        c32 = E.round_to(E.conv_pre(nchw(xin), oihw(wv), b, r, bool(relu), s, p, torch.float32), T)
        check_stored(nchw(y), ref, c32, tname, f"walk {what} {tuple(xin.shape)} -> {conv.out_channels}")
        nconv += 1
        return y

    for bi, blk in enumerate(E.trunk_blocks(orc)):
        main, down = E.block_convs(blk)
        out = step(main[0][0], x, None, 1, f"block {bi} conv1")
        identity = x
        if down is not None:
            identity = step(down[0], x, None, 0, f"block {bi} downsample")
        for j, (conv, _bn) in enumerate(main[1:]):
            last = j + 2 == len(main)
            out = step(conv, out, identity if last else None, 1, f"block {bi} conv{j + 2}")
        x = out
    N, Hf, Wf, Cf = x.shape
    feats = hip_avgpool(x.view(N, Hf * Wf, Cf), torch.full((N, Cf + 128), float("nan")), bf16)[:, :Cf]
    ref = E.avgpool(nchw(x), torch.float64)
    assert (feats.double() - ref).abs().max() <= 1e-6 * float(ref.abs().max())
    return feats.contiguous(), nconv


@pytest.mark.parametrize("tname", ["fp16", "bf16"])
@pytest.mark.parametrize("net,B,H,W", [("resnet34", 3, 88, 200), ("resnet34", 64, 88, 200),
                                       ("resnet50", 3, 176, 400), ("resnet50", 5, 88, 200)])
def test_infer16_network_layer_by_layer_then_bit_for_bit(net, B, H, W, tname):
    """(1) the engine's own 16-bit forward; (2) the walk: stem + 35 / 52 trunk convolutions, each
    pinned to one rounding at its real shape with the plan's folded weights and the previous HIP
    output as input; (3) the walk's pooled features equal the engine's `combined` BIT FOR BIT (pins
    the buffer rotation, the residual operands and the ReLU flags of trunk_fwd_eval16); (4) the fp32
    heads of the oracle on those features give the engine's outputs within 1e-4; (5) end to end,
    rms(HIP - emu64) on the pooled features <= 2 x rms(emu32 - emu64), the distance between two CPU
    realisations of the same rounded computation.

    Measured on an MI355X, HIP - emu64 on the pooled features, max / rms (beside emu32 - emu64):
      ResNet-34 B=3 88x200    fp16 1.58e-3 / 2.27e-4 (1.12e-3 / 2.23e-4)  bf16 1.23e-2 / 1.63e-3 (8.19e-3 / 1.43e-3)
      ResNet-34 B=64 88x200   fp16 1.95e-3 / 2.30e-4 (1.72e-3 / 2.27e-4)  bf16 1.40e-2 / 1.69e-3 (1.34e-2 / 1.53e-3)
      ResNet-50 B=3 176x400   fp16 3.38e-4 / 5.26e-5 (4.01e-4 / 5.07e-5)  bf16 2.80e-3 / 3.51e-4 (2.91e-3 / 3.55e-4)
      ResNet-50 B=5 88x200    fp16 5.66e-4 / 9.09e-5 (6.51e-4 / 9.14e-5)  bf16 4.46e-3 / 6.51e-4 (5.95e-3 / 6.42e-4)
    (max |feature| 4.2 .. 4.7); oracle heads on the HIP features vs the engine's outputs: <= 7.5e-7.
    """
    T = TYPES[tname][0]
    m, orc, eng, (img, spd, cmd), (c16, s16), view = _forward16(net, tname, B, H, W)
    x4, combined = view.io()
    assert torch.isfinite(x4).all() and (x4[..., :3].permute(0, 3, 1, 2) - img).abs().max() <= 1e-5
    numbers = _conv_numbers(orc)
    feats, nconv = _walk(orc, x4, lambda conv: view.folded(numbers[id(conv)]), tname)
    assert nconv == (35 if net == "resnet34" else 52)
    assert torch.equal(feats, combined), \
        f"walk != engine on {int((feats != combined).sum())} of {feats.numel()} pooled features"
    hc, hs = E.heads(orc, feats, spd, cmd)
    err = max(float((hc - c16).abs().max()), float((hs - s16).abs().max()))
    print(f"INFER16 {tname} {net} B={B} {H}x{W}: oracle heads on the HIP features vs engine outputs {err:.3e}")
    assert err <= TOL_OUT
    image = x4[..., :3].permute(0, 3, 1, 2).contiguous()       # the engine's own normalised image
    e64 = E.features(orc, image, T, torch.float64)
    e32 = E.features(orc, image, T, torch.float32).double()
    d_hip, d_cpu = feats.double() - e64, e32 - e64
    rms = lambda d: float(d.pow(2).mean().sqrt())
    print(f"INFER16 {tname} {net} B={B} {H}x{W}: HIP - emu64 max {float(d_hip.abs().max()):.3e} rms "
          f"{rms(d_hip):.3e}; emu32 - emu64 max {float(d_cpu.abs().max()):.3e} rms {rms(d_cpu):.3e}; "
          f"max|feature| {float(e64.abs().max()):.2f}")
    assert rms(d_hip) <= 2.0 * rms(d_cpu)


def test_infer16_report_largest_flip_shares():
    """Runs last in this file: the largest flip share per type over everything checked above."""
    for tname, v in _SHARES.items():
        if v:
            print(f"INFER16 largest flip share {tname}: {max(v):.3e} over {len(v)} tensors")
