"""Op-level fp32 parity of the implicit GEMM, its data gradient, the weight gradient and the fused
BatchNorm epilogues at the convolution shapes only the ResNet-50 variant (Bottleneck blocks) has:
stride-1 1x1 filters with 64 .. 2048 channels, 1x1 / stride 2 up to 1024 -> 2048, 3x3 / stride 2 with
Cin = Cout.  References, tolerances and helpers are those of tests/test_ops_gpu.py (torch's CPU
convolution and its autograd; 2e-5 of max(1, max|ref|) forward and data gradient, 3e-5 weight
gradient, 5e-5 plus the float64 yardstick above 10,000 pixels) and, for the column partials, the
float64 gates of tests/test_conv_classes_gpu.py.

Where a test is about a branch of the launchers it first PROVES that the launch takes it, through
cilrs_conv2d_plan_info (the launchers' own decision code), the *nblk a fused call reports, or the
weight gradient's scratch size -- a failed regime assertion means the case list is stale, not that
a kernel is wrong:

  wide split-K reduce        test_fwd_stats / test_dgrad_bnbwd with force_splitk = 2: 1,024 written
                             columns keep the column partials (*nblk > 0), 2,048 go to the plain
                             reduce (*nblk == 0, partial buffer untouched)
  stride-1 1x1, K loops of   BOTTLENECK_F32_CASES through every forced tile and split; 128- and 64-row
  2 .. 64 K-tiles            fused partials (*nblk == cdiv(M, 128) / cdiv(M, 64))
  separate parity launches   test_dgrad_stride2_parity_launches: parity_fused == 0 under the
                             automatic plan on odd maps, next to a fused sibling just under the limit
  one-tile weight gradient   test_wgrad_single_tile_many_slabs: one tile of output, >= 128 slabs
  position classes, 512      test_classes_512_channels_6x13: class_tiles > 0, nine classes, split 2
  channels, 6x13             with scratch and unsplit without
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import test_ops_gpu as T
from test_conv_classes_gpu import NO_CLASSES, _EPS, _ROWS, _col_sums
from test_ops_gpu import _lib, _tol, _wgrad_vs_f64, dev, nhwc, ohwi, stream

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (N, H, W, Cin, Cout, k, stride, pad): the Bottleneck layers on the maps of an 88x200 frame
BOTTLENECK_F32_CASES = [
    (2, 22, 50, 64, 64, 1, 1, 0),        # layer1 conv1 of block 0: the shortest K loop (2 K-tiles)
    (2, 22, 50, 64, 256, 1, 1, 0),       # layer1 conv3 and the stride-1 down-sample
    (2, 22, 50, 256, 64, 1, 1, 0),       # layer1 conv1
    (2, 22, 50, 256, 128, 1, 1, 0),      # layer2.0 conv1
    (2, 22, 50, 128, 128, 3, 2, 1),      # layer2.0 conv2: 3x3 / stride 2 with Cin = Cout
    (2, 22, 50, 256, 512, 1, 2, 0),      # layer2.0 down-sample
    (3, 11, 25, 128, 512, 1, 1, 0),
    (3, 11, 25, 512, 128, 1, 1, 0),
    (3, 11, 25, 512, 256, 1, 1, 0),
    (3, 11, 25, 256, 256, 3, 2, 1),
    (3, 11, 25, 512, 1024, 1, 2, 0),
    (5, 6, 13, 256, 1024, 1, 1, 0),      # 1,024 written columns: the widest that keeps the cols reduce
    (5, 6, 13, 1024, 256, 1, 1, 0),
    (5, 6, 13, 1024, 512, 1, 1, 0),
    (5, 6, 13, 512, 512, 3, 2, 1),
    (5, 6, 13, 1024, 2048, 1, 2, 0),
    (7, 3, 7, 512, 2048, 1, 1, 0),       # 2,048 written columns
    (7, 3, 7, 2048, 512, 1, 1, 0),       # the longest 1x1 K loop (64 K-tiles)
    (1, 3, 7, 2048, 512, 1, 1, 0),       # single frame (M = 21)
]
STRIDE2 = [c for c in BOTTLENECK_F32_CASES if c[6] == 2]
ONE_BY_ONE_S2 = [c for c in STRIDE2 if c[5] == 1]
# the fused BatchNorm epilogues are stride 1: the 1x1 cases above and layer4's 3x3
STRIDE1 = [c for c in BOTTLENECK_F32_CASES if c[6] == 1] + [(7, 3, 7, 512, 512, 3, 1, 1)]


def _id(case):
    N, H, W, Cin, Cout, k, s, p = case
    return f"n{N}_{H}x{W}_{Cin}to{Cout}_k{k}s{s}"


def _matrix(test, names):
    """the parametrisation `names` of a test of tests/test_ops_gpu.py: the same matrix, not a copy"""
    return next(m.args[1] for m in test.pytestmark if m.name == "parametrize" and m.args[0] == names)


FWD_PLANS = _matrix(T.test_conv_fwd, "cfg,splitk")
DGRAD_PLANS = sorted({(cfg, sk) for cfg, sk, _ in _matrix(T.test_conv_dgrad, "cfg,splitk,with_addend")})


def cdiv(a, b):
    return -(-a // b)


def out_hw(case):
    N, H, W, Cin, Cout, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def plan_info(case, dgrad, scratch_floats, cfg=-1, splitk=0):
    """what the launcher would run: cfg, splitk, class_tiles, parity_fused"""
    L = _lib()
    out = [C.c_int(-9) for _ in range(4)]
    L.check(L.lib().cilrs_conv2d_plan_info(*case, int(dgrad), scratch_floats, cfg, splitk,
                                           *[C.byref(v) for v in out]))
    return SimpleNamespace(cfg=out[0].value, splitk=out[1].value, class_tiles=out[2].value,
                           parity_fused=out[3].value)


def tile_rows(cfg):
    return 128 if cfg in (0, 1, 3, 4) else 64


_cache = {}


def _data(case, seed=41):
    """Inputs and torch references of a case, computed once and never modified: x, w (scaled to
    unit output variance), y = conv(x, w), dy, dx = dgrad(dy), an addend of dx's shape (NHWC)."""
    if case not in _cache:
        N, H, W, Cin, Cout, k, s, p = case
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(N, Cin, H, W, generator=g, requires_grad=True)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
        y = F.conv2d(x, w, None, s, p)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        add = torch.randn(N, H, W, Cin, generator=g)
        _cache[case] = SimpleNamespace(x=x.detach(), w=w, y=y.detach(), dy=dy, dx=x.grad.detach(),
                                       add=add)
    return _cache[case]


def _close(got, want, what, scale=2e-5):
    assert torch.isfinite(got).all(), what
    err, tol = float((got - want).abs().max()), _tol(want, scale)
    print(f"{what}: max err {err:.3e} (tol {tol:.3e})")
    assert err <= tol, what


# ---- a. the Bottleneck shapes at small batch --------------------------------------------------------
@pytest.mark.parametrize("cfg,splitk", FWD_PLANS)
@pytest.mark.parametrize("case", BOTTLENECK_F32_CASES, ids=_id)
def test_conv_fwd(case, cfg, splitk):
    L = _lib()
    N, H, W, Cin, Cout, k, s, p = case
    if cfg in (0, 3) and Cout % 128:
        pytest.skip("128-wide tile needs Cout % 128 == 0")
    d = _data(case)
    Ho, Wo = out_hw(case)
    y = torch.full((N, Ho, Wo, Cout), NAN, device="cuda")
    scratch = torch.empty(8 * y.numel(), device="cuda")
    xd, wd = nhwc(d.x), ohwi(d.w)
    L.check(L.lib().cilrs_conv2d_fwd(L.ptr(xd), L.ptr(wd), L.ptr(y), N, H, W, Cin, Cout, k, k, s, p,
                                     cfg, splitk, L.ptr(scratch), scratch.numel(), stream()))
    torch.cuda.synchronize()
    _close(y.cpu().permute(0, 3, 1, 2), d.y, f"fwd {case} cfg {cfg} split {splitk}")


def _unreached_equal(case, got, held):
    """1x1 / stride 2, pad 0: only the pixels (even row, even column) see a filter tap; every other
    pixel of dx is bit-identical to `held` (what it held before, the addend, or zero)"""
    assert case[5] == 1 and case[6] == 2 and case[7] == 0
    assert torch.equal(got[:, 1::2], held[:, 1::2])
    assert torch.equal(got[:, ::2, 1::2], held[:, ::2, 1::2])


def _dgrad(case, dyd, wd, dx, addend, cfg, splitk, scratch):
    L = _lib()
    N, H, W, Cin, Cout, k, s, p = case
    L.check(L.lib().cilrs_conv2d_dgrad(L.ptr(dyd), L.ptr(wd), L.ptr(dx), L.ptr(addend), N, H, W, Cin,
                                       Cout, k, k, s, p, cfg, splitk, L.ptr(scratch),
                                       scratch.numel() if scratch is not None else 0, stream()))
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("cfg,splitk", DGRAD_PLANS)
@pytest.mark.parametrize("case", BOTTLENECK_F32_CASES, ids=_id)
def test_conv_dgrad(case, cfg, splitk):
    """plain and with an addend under every plan of test_ops_gpu.test_conv_dgrad"""
    N, H, W, Cin, Cout, k, s, p = case
    d = _data(case)
    dyd, wd, addd = nhwc(d.dy), ohwi(d.w), dev(d.add)
    want = d.dx.permute(0, 2, 3, 1)
    scratch = torch.empty(8 * want.numel(), device="cuda")
    for addend, ref, held in ((None, want, torch.zeros_like(d.add)), (addd, want + d.add, d.add)):
        dx = torch.full((N, H, W, Cin), NAN, device="cuda")
        got = _dgrad(case, dyd, wd, dx, addend, cfg, splitk, scratch)
        _close(got, ref, f"dgrad {case} cfg {cfg} split {splitk} addend {addend is not None}")
        if case in ONE_BY_ONE_S2:
            _unreached_equal(case, got, held)


@pytest.mark.parametrize("case", STRIDE2, ids=_id)
def test_conv_dgrad_stride2_in_place(case):
    """dx += dgrad(dy) with addend == dx, as test_ops_gpu.test_conv_dgrad_stride2_in_place: parity
    classes no tap reaches get no blocks and keep their bits"""
    d = _data(case)
    dyd, wd = nhwc(d.dy), ohwi(d.w)
    dx = dev(d.add.clone())
    scratch = torch.empty(8 * dx.numel(), device="cuda")
    assert plan_info(case, True, scratch.numel()).parity_fused == 1      # (small batch: one launch)
    got = _dgrad(case, dyd, wd, dx, dx, -1, 0, scratch)
    _close(got, d.dx.permute(0, 2, 3, 1) + d.add, f"dgrad in place {case}")
    if case in ONE_BY_ONE_S2:
        _unreached_equal(case, got, d.add)


def _wgrad_f64(case, x, dy):
    N, H, W, Cin, Cout, k, s, p = case
    w64 = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, s, p).backward(dy.double())
    return w64.grad.permute(0, 2, 3, 1)


def _wgrad(case, x, dy):
    """(dw as the kernel wrote it [Cout][k][k][Cin], slabs the plan sums)"""
    L = _lib()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    nsc = lib.cilrs_conv2d_wgrad_scratch_floats(N, H, W, Cin, Cout, k, k, s, p)
    assert nsc % (Cout * k * k * Cin) == 0
    scratch = torch.full((nsc,), NAN, device="cuda")
    dw = torch.full((Cout, k, k, Cin), NAN, device="cuda")
    xd, dyd = nhwc(x), nhwc(dy)
    L.check(lib.cilrs_conv2d_wgrad(L.ptr(xd), L.ptr(dyd), L.ptr(dw), L.ptr(scratch), N, H, W, Cin,
                                   Cout, k, k, s, p, Cin, stream()))
    torch.cuda.synchronize()
    return dw.cpu(), nsc // (Cout * k * k * Cin)


@pytest.mark.parametrize("case", BOTTLENECK_F32_CASES, ids=_id)
def test_conv_wgrad(case):
    """Against the float64 weight gradient.  Slabs the plan sums, read from the scratch size (stride
    1 / stride 2 cases): 14 / 4 on the 22x50 maps, 6 / 2 on 11x25, 3 or 2 / 1 on 6x13, 1 on 3x7.  The
    two shapes with the most tiles and the fewest splits of the variant, (5,6,13,1024,2048,1,2,0)
    and (7,3,7,2048,512,1,1,0), are ONE-slab launches: the reduce copies a single slab (pinned by
    test_wgrad_split_counts_of_the_widest_layers)."""
    d = _data(case)
    got, splits = _wgrad(case, d.x, d.dy)
    print(f"wgrad {case}: {splits} slabs")
    assert splits >= 1
    _close(got.double(), _wgrad_f64(case, d.x, d.dy), f"wgrad {case}", 3e-5)


def test_wgrad_split_counts_of_the_widest_layers():
    """what test_conv_wgrad's docstring records: both are one-slab launches"""
    lib = _lib().lib()
    for case in [(5, 6, 13, 1024, 2048, 1, 2, 0), (7, 3, 7, 2048, 512, 1, 1, 0)]:
        N, H, W, Cin, Cout, k, s, p = case
        assert lib.cilrs_conv2d_wgrad_scratch_floats(N, H, W, Cin, Cout, k, k, s, p) == Cout * k * k * Cin


# ---- b. fused BatchNorm epilogues --------------------------------------------------------------------
# (cfg, splitk): a 128-row tile and the 64-row tile unsplit, the automatic plan, two forced slabs
STATS_PLANS = [(1, 1), (2, 1), (-1, 0), (-1, 2)]


def _pattern(n):
    return (torch.arange(n, device="cuda") % 977).float() + 0.5


def _expect_nblk(case, dgrad, scratch_floats, cfg, splitk, nblk):
    """*nblk against the plan the query reports; returns whether the partials are fused"""
    N, H, W, Cin, Cout, k, s, p = case
    M, cols = (N * H * W, Cin) if dgrad else (N * out_hw(case)[0] * out_hw(case)[1], Cout)
    plan = plan_info(case, dgrad, scratch_floats, cfg, splitk)
    print(f"  plan {case} dgrad {int(dgrad)} forced ({cfg}, {splitk}): cfg {plan.cfg} split "
          f"{plan.splitk} class tiles {plan.class_tiles}; nblk {nblk}")
    if cfg >= 0:
        assert plan.cfg == cfg
    if splitk > 0:
        assert plan.splitk == splitk
    if plan.splitk == 1:
        if plan.class_tiles:
            assert nblk == plan.class_tiles // (cols // 64)
        else:
            assert nblk == cdiv(M, tile_rows(plan.cfg))
    elif cols <= 1024:
        assert 0 < nblk <= 1024             # the split-K reduce emits them
    else:
        assert nblk == 0                    # too wide for the column reduce: plain reduce, not fused
    return nblk > 0


def _fwd_stats(case, cfg, splitk, with_scratch=True):
    """cilrs_conv2d_fwd_stats -> (y [M][Cout] on the host, fused?)"""
    L = _lib()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    d = _data(case)
    Ho, Wo = out_hw(case)
    M = N * Ho * Wo
    xd, wd = nhwc(d.x), ohwi(d.w)
    y = torch.full((M, Cout), NAN, device="cuda")
    part = _pattern(lib.cilrs_bn_partial_floats(Cout))
    part0 = part.clone()
    scratch = torch.empty(8 * y.numel(), device="cuda") if with_scratch else None
    floats = scratch.numel() if with_scratch else 0
    nblk = C.c_int(-1)
    L.check(lib.cilrs_conv2d_fwd_stats(L.ptr(xd), L.ptr(wd), L.ptr(y), L.ptr(part), C.byref(nblk), N,
                                       H, W, Cin, Cout, k, s, p, cfg, splitk, L.ptr(scratch), floats,
                                       stream()))
    torch.cuda.synchronize()
    fused = _expect_nblk(case, False, floats, cfg, splitk, nblk.value)
    yc = y.cpu()
    _close(yc, d.y.permute(0, 2, 3, 1).reshape(M, Cout), f"fwd_stats {case} ({cfg}, {splitk})")
    if not fused:
        assert torch.equal(part, part0), "partial buffer written although *nblk == 0"
        return yc, False
    # the float64 gates of test_conv_classes_gpu.test_conv_fwd_classes_bn_partials: partials summed
    # over the row groups against the column sums of the stored y (one rounding per squared term)
    assert torch.equal(part[2 * Cout * nblk.value:], part0[2 * Cout * nblk.value:])
    s1, s2 = _col_sums(part, nblk.value, Cout)
    assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
    y64 = yc.double()
    x1 = float((s1 - y64.sum(0)).abs().max())
    x2 = float((s2 - (y64 * y64).sum(0)).abs().max())
    t1 = _ROWS * _EPS * float(y64.abs().sum(0).max())
    t2 = (_ROWS + 1) * _EPS * float((y64 * y64).sum(0).max())
    print(f"  partials vs float64: sum err {x1:.3e} (tol {t1:.3e}) sum sq err {x2:.3e} (tol {t2:.3e})")
    assert x1 <= t1 and x2 <= t2
    return yc, True


@pytest.mark.parametrize("cfg,splitk", STATS_PLANS)
@pytest.mark.parametrize("case", STRIDE1, ids=_id)
def test_fwd_stats(case, cfg, splitk):
    """y and the forward column partials; *nblk == cdiv(M, 128) / cdiv(M, 64) unsplit, > 0 from the
    split-K reduce up to 1,024 columns, 0 (and the buffer untouched) at 2,048"""
    _, fused = _fwd_stats(case, cfg, splitk)
    if splitk == 2:
        assert fused == (case[4] <= 1024)


_bn_cache = {}


def _bn_state(M, Cc, relu):
    """the BatchNorm layer whose output gradient dx is: raw input yb, output z, statistics (mean |
    rstd | ...) from cilrs_bn_train_fwd, as test_conv_dgrad_classes_bn_bwd_partials sets it up"""
    key = (M, Cc, relu)
    if key not in _bn_cache:
        L = _lib()
        lib = L.lib()
        g = torch.Generator().manual_seed(12)
        yb = (torch.randn(M, Cc, generator=g) * 1.3 + 0.2).cuda()
        gamma = (torch.rand(Cc, generator=g) + 0.5).cuda()
        beta = (torch.rand(Cc, generator=g) - 0.5).cuda()
        rm, rv = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        stats = torch.empty(4 * Cc, device="cuda")
        part = torch.empty(lib.cilrs_bn_partial_floats(Cc), device="cuda")
        z = torch.empty(M, Cc, device="cuda")
        L.check(lib.cilrs_bn_train_fwd(L.ptr(yb), M, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv),
                                       L.ptr(nbt), 0.1, 1e-5, None, relu, L.ptr(stats), L.ptr(part),
                                       L.ptr(z), stream()))
        torch.cuda.synchronize()
        _bn_cache[key] = (yb.cpu(), z.cpu(), stats.cpu())
    return _bn_cache[key]


def _dgrad_bnbwd(case, relu, cfg, splitk, with_scratch=True):
    """cilrs_conv2d_dgrad_bnbwd (with an addend) -> (dx [M][Cin] on the host, fused?)"""
    L = _lib()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    d = _data(case)
    M = N * H * W
    yb, z, stats = _bn_state(M, Cin, relu)
    ybd, zd, statsd = dev(yb), dev(z), dev(stats)
    dyd, wd, addd = nhwc(d.dy), ohwi(d.w), dev(d.add)
    dx = torch.full((M, Cin), NAN, device="cuda")
    part = _pattern(lib.cilrs_bn_partial_floats(Cin))
    part0 = part.clone()
    scratch = torch.empty(8 * dx.numel(), device="cuda") if with_scratch else None
    floats = scratch.numel() if with_scratch else 0
    nblk = C.c_int(-1)
    L.check(lib.cilrs_conv2d_dgrad_bnbwd(L.ptr(dyd), L.ptr(wd), L.ptr(dx), L.ptr(addd), L.ptr(zd),
                                         L.ptr(ybd), L.ptr(statsd), relu, L.ptr(part), C.byref(nblk),
                                         N, H, W, Cin, Cout, k, s, p, cfg, splitk, L.ptr(scratch),
                                         floats, stream()))
    torch.cuda.synchronize()
    fused = _expect_nblk(case, True, floats, cfg, splitk, nblk.value)
    dxc = dx.cpu()
    want = (d.dx.permute(0, 2, 3, 1) + d.add).reshape(M, Cin)
    _close(dxc, want, f"dgrad_bnbwd {case} relu {relu} ({cfg}, {splitk})")
    if not fused:
        assert torch.equal(part, part0), "partial buffer written although *nblk == 0"
        return dxc, False
    # the float64 gates of test_conv_dgrad_classes_bn_bwd_partials on the stored dx: g = dx * (z > 0)
    # is exact, xhat = (y - mean) * rstd takes two roundings in fp32 and the product one
    assert torch.equal(part[2 * Cin * nblk.value:], part0[2 * Cin * nblk.value:])
    s1, s2 = _col_sums(part, nblk.value, Cin)
    assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
    gg = dxc.double() * (z > 0) if relu else dxc.double()
    st = stats.double()
    xhat = (yb.double() - st[:Cin]) * st[Cin:2 * Cin]
    x1 = float((s1 - gg.sum(0)).abs().max())
    x2 = float((s2 - (gg * xhat).sum(0)).abs().max())
    t1 = _ROWS * _EPS * float(gg.abs().sum(0).max())
    t2 = (_ROWS + 3) * _EPS * float((gg * xhat).abs().sum(0).max())
    print(f"  partials vs float64: sum g err {x1:.3e} (tol {t1:.3e}) sum g xhat err {x2:.3e} (tol {t2:.3e})")
    assert x1 <= t1 and x2 <= t2
    return dxc, True


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("cfg,splitk", STATS_PLANS)
@pytest.mark.parametrize("case", STRIDE1, ids=_id)
def test_dgrad_bnbwd(case, cfg, splitk, relu):
    """dx and the BatchNorm-backward partials (sum g, sum g * xhat); the written columns are the
    forward Cin: fused from the split-K reduce up to 1,024 of them, not at 2,048"""
    _, fused = _dgrad_bnbwd(case, relu, cfg, splitk)
    if splitk == 2:
        assert fused == (case[3] <= 1024)


# ---- c. plan regimes of the ResNet-50 benchmark leg, at the smallest shapes that reach them ---------
# stride-2 data gradient: one launch while cdiv(N * ceil(H/2) * ceil(W/2), 64) * (Cin / 64) < 1280, four
# launches with the cost model's own tile and split per parity class from there on.  Odd maps: the
# four classes have 51x52, 51x51, 50x52 and 50x51 pixels.  (1,328 / 1,276 and 1,328 / 1,264 tiles)
PARITY_CASES = [
    ((8, 101, 103, 256, 256, 3, 2, 1), 0),
    ((8, 101, 99, 256, 256, 3, 2, 1), 1),
    ((2, 101, 103, 1024, 2048, 1, 2, 0), 0),
    ((2, 101, 97, 1024, 2048, 1, 2, 0), 1),
]


@pytest.mark.parametrize("case,fused", PARITY_CASES, ids=[_id(c) + ("_fused" if f else "_separate")
                                                          for c, f in PARITY_CASES])
def test_dgrad_stride2_parity_launches(case, fused):
    """automatic plan (force_cfg -1, force_splitk 0) on both sides of the limit, same generator:
    plain, with an addend, and in place"""
    N, H, W, Cin, Cout, k, s, p = case
    from cilrs_mi355.hostinfo import usable_cores
    torch.set_num_threads(usable_cores())
    g = torch.Generator().manual_seed(43)
    x = torch.randn(N, Cin, H, W, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
    y = F.conv2d(x, w, None, s, p)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    want = x.grad.permute(0, 2, 3, 1)
    add = torch.randn(N, H, W, Cin, generator=g)
    dyd, wd, addd = nhwc(dy), ohwi(w), dev(add)
    scratch = torch.empty(8 * add.numel(), device="cuda")
    plan = plan_info(case, True, scratch.numel())
    print(f"parity {case}: fused {plan.parity_fused}, cfg {plan.cfg}, split {plan.splitk}")
    assert plan.parity_fused == fused
    dx = torch.full((N, H, W, Cin), NAN, device="cuda")
    acc = addd.clone()                     # in place: the addend IS dx
    for name, buf, addend, ref, held in (("plain", dx, None, want, torch.zeros_like(add)),
                                         ("addend", dx.clone(), addd, want + add, add),
                                         ("in place", acc, acc, want + add, add)):
        got = _dgrad(case, dyd, wd, buf, addend, -1, 0, scratch)
        _close(got, ref, f"parity {case} {name}")
        if k == 1:
            _unreached_equal(case, got, held)


@pytest.mark.parametrize("case", [(8, 44, 100, 64, 64, 1, 1, 0), (8, 44, 100, 64, 256, 1, 1, 0),
                                  (8, 44, 100, 256, 64, 1, 1, 0)], ids=_id)
def test_wgrad_single_tile_many_slabs(case):
    """1x1 64 -> 64 is ONE 64x64 tile of output: the split count is bounded by the pixel count alone
    (220 slabs at 35,200 pixels), and the slab reduce runs with 16 thread groups per output
    (8 x 16 <= slabs).  Its two neighbours have four tiles (or one 128-wide pair) and 123 slabs."""
    N, H, W, Cin, Cout, k, s, p = case
    g = torch.Generator().manual_seed(44)
    x = torch.randn(N, Cin, H, W, generator=g)
    dy = torch.randn(N, Cout, H, W, generator=g)
    got, splits = _wgrad(case, x, dy)
    print(f"wgrad {case}: {splits} slabs")
    if Cin == 64 and Cout == 64:
        assert Cout * k * k * Cin == 64 * 64 and splits >= 128
    w32 = torch.zeros(Cout, Cin, k, k, requires_grad=True)
    F.conv2d(x, w32, None, s, p).backward(dy)
    cpu32 = w32.grad.permute(0, 2, 3, 1)
    _close(got, cpu32, f"wgrad {case}", 5e-5)
    _wgrad_vs_f64(x, dy, (Cout, Cin, k, k), s, p, got, cpu32)


CLASSES_512 = (64, 6, 13, 512, 512, 3, 1, 1)      # ResNet-50's layer4 conv2 at 176x400, half the batch


@pytest.mark.parametrize("with_scratch", [True, False], ids=["split", "unsplit"])
def test_classes_512_channels_6x13_fwd(with_scratch):
    """Nine position classes with a 144 K-tile loop: right against torch, the column partials right,
    and the bits of the single launch (force_cfg = -2)."""
    case = CLASSES_512
    y = 8 * 64 * 78 * 512 if with_scratch else 0
    plan = plan_info(case, False, y)
    assert plan.class_tiles > 0 and plan.cfg == 2 and plan.splitk == (2 if with_scratch else 1)
    assert plan_info(case, False, y, NO_CLASSES).class_tiles == 0
    on, _ = _fwd_stats(case, -1, 0, with_scratch)
    off, _ = _fwd_stats(case, NO_CLASSES, 0, with_scratch)
    assert torch.equal(on, off)


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("with_scratch", [True, False], ids=["split", "unsplit"])
def test_classes_512_channels_6x13_dgrad(with_scratch, relu):
    case = CLASSES_512
    dx = 8 * 64 * 78 * 512 if with_scratch else 0
    plan = plan_info(case, True, dx)
    assert plan.class_tiles > 0 and plan.cfg == 2 and plan.splitk == (2 if with_scratch else 1)
    on, _ = _dgrad_bnbwd(case, relu, -1, 0, with_scratch)
    off, _ = _dgrad_bnbwd(case, relu, NO_CLASSES, 0, with_scratch)
    assert torch.equal(on, off)
