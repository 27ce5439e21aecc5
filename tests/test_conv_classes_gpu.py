"""Position classes of the implicit GEMM (csrc/conv_igemm.hip): a padded stride-1 map whose every
class has at least a tile of rows runs as corner / edge / interior rectangles in ONE launch, each
with only the filter taps that meet the image, split-K kept.

Reference and tolerance are those of test_conv_fwd / test_conv_dgrad in tests/test_ops_gpu.py
(torch fp32 CPU convolution, 2e-5 of max(1, max|ref|)).  Every case is also run with the class
launch switched off for that call (force_cfg = -2: automatic choice, single problem) and twice
with it on: on and on are bit-identical, and so are on and off -- a class launch keeps the single
problem's split count and K ranges and only drops products with padding.

The fused BatchNorm reductions get cases of their own: a wrong global tile index or pixel map
would leave y right and the column partials wrong."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NO_CLASSES = -2        # force_cfg: the automatic choice without the class launch


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def ohwi(w):
    return w.permute(0, 2, 3, 1).contiguous().cuda()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tol(ref, scale=2e-5):
    return scale * max(1.0, float(ref.abs().max()))


# (N, H, W, Cin, Cout, force_splitk, scratch given) -- all 3x3 / stride 1 / pad 1
CASES = [
    (64, 3, 7, 64, 64, 0, False),      # one whole tile per corner class, no split
    (64, 3, 7, 64, 64, 2, True),       # split-K slabs: dense images of the whole output
    (64, 3, 7, 64, 64, 3, True),
    (72, 3, 7, 64, 128, 0, False),     # a partial second tile in every class
    (64, 1, 7, 64, 64, 0, False),      # only the middle filter row valid: three classes
    (64, 2, 2, 64, 64, 0, False),      # four corner classes, no interior
    (64, 6, 13, 64, 64, 0, False),     # nine classes with a large interior
]
_IDS = ["n64_3x7", "n64_3x7_split2", "n64_3x7_split3", "n72_3x7_c128", "n64_1x7", "n64_2x2",
        "n64_6x13"]

_data_cache = {}


def _data(case):
    """Inputs and torch references of a case, computed once: x, w, y = conv(x, w), dy, dx."""
    if case not in _data_cache:
        N, H, W, Cin, Cout = case[:5]
        g = torch.Generator().manual_seed(11)
        x = torch.randn(N, Cin, H, W, generator=g, requires_grad=True)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        y = F.conv2d(x, w, None, 1, 1)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        add = torch.randn(N, H, W, Cin, generator=g)
        _data_cache[case] = (x.detach(), w, y.detach(), dy, x.grad.detach(), add)
    return _data_cache[case]


def _takes(case, dgrad):
    L = _lib()
    N, H, W, Cin, Cout, splitk, with_scratch = case
    rows = N * H * W
    floats = 8 * rows * (Cin if dgrad else Cout) if with_scratch else 0
    return L.lib().cilrs_conv2d_takes_classes(N, H, W, Cin, Cout, 3, 1, 1, int(dgrad), floats, splitk)


def _fwd(case, xd, wd, cfg):
    L = _lib()
    N, H, W, Cin, Cout, splitk, with_scratch = case
    y = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    scratch = torch.empty(8 * y.numel(), device="cuda") if with_scratch else None
    L.check(L.lib().cilrs_conv2d_fwd(L.ptr(xd), L.ptr(wd), L.ptr(y), N, H, W, Cin, Cout, 3, 3, 1, 1,
                                     cfg, splitk, L.ptr(scratch),
                                     scratch.numel() if with_scratch else 0, stream()))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_conv_fwd_classes(case):
    x, w, ref, _, _, _ = _data(case)
    assert _takes(case, False) == 1, "the case must take the class launch"
    xd, wd = nhwc(x), ohwi(w)
    want = ref.permute(0, 2, 3, 1)
    on = _fwd(case, xd, wd, -1)
    on2 = _fwd(case, xd, wd, -1)
    off = _fwd(case, xd, wd, NO_CLASSES)
    for name, got in (("classes", on), ("single", off)):
        assert torch.isfinite(got).all(), name
        err = float((got - want).abs().max())
        print(f"fwd {case} {name}: max err {err:.3e} (tol {_tol(want):.3e})")
        assert err <= _tol(want), name
    assert float((on - off).abs().max()) <= _tol(want)
    assert torch.equal(on, off)      # same split, same K ranges, only products with padding dropped
    assert torch.equal(on, on2)


def _dgrad(case, dyd, wd, addend, cfg, in_place=False):
    L = _lib()
    N, H, W, Cin, Cout, splitk, with_scratch = case
    if in_place:
        dx = addend.clone()
        addend = dx
    else:
        dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
    scratch = torch.empty(8 * dx.numel(), device="cuda") if with_scratch else None
    L.check(L.lib().cilrs_conv2d_dgrad(L.ptr(dyd), L.ptr(wd), L.ptr(dx), L.ptr(addend), N, H, W, Cin,
                                       Cout, 3, 3, 1, 1, cfg, splitk, L.ptr(scratch),
                                       scratch.numel() if with_scratch else 0, stream()))
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_conv_dgrad_classes(case, with_addend):
    _, w, _, dy, ref, add = _data(case)
    assert _takes(case, True) == 1, "the case must take the class launch"
    dyd, wd = nhwc(dy), ohwi(w)
    addd = add.cuda() if with_addend else None
    want = ref.permute(0, 2, 3, 1)
    if with_addend:
        want = want + add
    on = _dgrad(case, dyd, wd, addd, -1)
    on2 = _dgrad(case, dyd, wd, addd, -1)
    off = _dgrad(case, dyd, wd, addd, NO_CLASSES)
    for name, got in (("classes", on), ("single", off)):
        assert torch.isfinite(got).all(), name
        err = float((got - want).abs().max())
        print(f"dgrad {case} addend={with_addend} {name}: max err {err:.3e} (tol {_tol(want):.3e})")
        assert err <= _tol(want), name
    assert float((on - off).abs().max()) <= _tol(want)
    assert torch.equal(on, off)      # same split, same K ranges, only products with padding dropped
    assert torch.equal(on, on2)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[_IDS[0], _IDS[1], _IDS[3]])
def test_conv_dgrad_classes_addend_in_place(case):
    """dx += dgrad(dy): the addend IS dx (the residual join of a BasicBlock)."""
    _, w, _, dy, ref, add = _data(case)
    dyd, wd = nhwc(dy), ohwi(w)
    want = ref.permute(0, 2, 3, 1) + add
    on = _dgrad(case, dyd, wd, add.cuda(), -1, in_place=True)
    on2 = _dgrad(case, dyd, wd, add.cuda(), -1, in_place=True)
    off = _dgrad(case, dyd, wd, add.cuda(), NO_CLASSES, in_place=True)
    assert float((on - want).abs().max()) <= _tol(want)
    assert float((on - off).abs().max()) <= _tol(want)
    assert torch.equal(on, off)      # same split, same K ranges, only products with padding dropped
    assert torch.equal(on, on2)


# ---- fused BatchNorm reductions -------------------------------------------------------------------
# fp32 sums of M terms in a fixed but arbitrary order: either side is within (M - 1) eps sum|t| / 2
# of the exact sum (eps = 2^-23), so two orders differ by at most M eps sum|t|.
_EPS = 2.0 ** -23
# The fused partials themselves sum at most 64 rows in fp32 (a 64-row tile; 16 rows per block of the
# slab reduce at these shapes) and the test adds the partials in float64, so against the float64
# sum of the stored tensor they are within (64 + r) eps sum|t|, r = roundings that form a term.
_ROWS = 64
FUSED = [CASES[0], CASES[1]]          # N = 64, 3x7, C = 64: without and with split


def _col_sums(partial, nblk, Cc):
    p = partial[: 2 * Cc * nblk].double().cpu().view(2, Cc, nblk).sum(-1)
    return p[0], p[1]


@pytest.mark.parametrize("cfg", [-1, NO_CLASSES], ids=["classes", "single"])
@pytest.mark.parametrize("case", FUSED, ids=["nosplit", "split2"])
def test_conv_fwd_classes_bn_partials(case, cfg):
    """Column partials of the forward epilogue (unsplit: per tile, the tile index running over all
    classes; split: by the slab reduce), finalised, against cilrs_bn_train_stats on the stored y."""
    L = _lib()
    lib = L.lib()
    N, H, W, Cin, Cout, splitk, with_scratch = case
    x, w, _, _, _, _ = _data(case)
    M = N * H * W
    xd, wd = nhwc(x), ohwi(w)
    y = torch.full((M, Cout), float("nan"), device="cuda")
    part = torch.full((lib.cilrs_bn_partial_floats(Cout),), float("nan"), device="cuda")
    scratch = torch.empty(8 * y.numel(), device="cuda") if with_scratch else None
    nblk = C.c_int(-1)
    L.check(lib.cilrs_conv2d_fwd_stats(L.ptr(xd), L.ptr(wd), L.ptr(y), L.ptr(part), C.byref(nblk),
                                       N, H, W, Cin, Cout, 3, 1, 1, cfg, splitk, L.ptr(scratch),
                                       scratch.numel() if with_scratch else 0, stream()))
    torch.cuda.synchronize()
    assert nblk.value > 0
    if cfg == -1 and splitk <= 1:
        assert nblk.value == 21            # 4 + 2 corner / end tiles, 3 x 5 edge / interior tiles
    s1, s2 = _col_sums(part, nblk.value, Cout)
    assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
    mean = s1 / M
    var = (s2 - M * mean * mean) / (M - 1)
    acc = torch.zeros(2 + 4 * Cout, dtype=torch.float64, device="cuda")
    part2 = torch.empty(lib.cilrs_bn_partial_floats(Cout), device="cuda")
    L.check(lib.cilrs_bn_train_stats(L.ptr(y), M, Cout, L.ptr(acc), L.ptr(part2), stream()))
    torch.cuda.synchronize()
    a = acc.cpu()
    ref_mean, ref_var = a[2:2 + Cout], a[2 + Cout:2 + 2 * Cout]
    yc = y.double().cpu()
    tol_mean = _EPS * float(yc.abs().sum(0).max())                 # M eps sum|y| / M
    tol_var = _EPS * float((yc * yc).sum(0).max()) * M / (M - 1) + 2 * float(mean.abs().max()) * tol_mean
    e_mean, e_var = float((mean - ref_mean).abs().max()), float((var - ref_var).abs().max())
    print(f"bn partials {case} cfg {cfg}: nblk {nblk.value} mean err {e_mean:.3e} (tol {tol_mean:.3e}) "
          f"var err {e_var:.3e} (tol {tol_var:.3e})")
    assert e_mean <= tol_mean and e_var <= tol_var
    # and against the float64 column sums of the stored y (one rounding per squared term)
    x1 = float((s1 - yc.sum(0)).abs().max())
    x2 = float((s2 - (yc * yc).sum(0)).abs().max())
    t1 = _ROWS * _EPS * float(yc.abs().sum(0).max())
    t2 = (_ROWS + 1) * _EPS * float((yc * yc).sum(0).max())
    print(f"  vs float64: sum err {x1:.3e} (tol {t1:.3e}) sum sq err {x2:.3e} (tol {t2:.3e})")
    assert x1 <= t1 and x2 <= t2


@pytest.mark.parametrize("cfg", [-1, NO_CLASSES], ids=["classes", "single"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("case", FUSED, ids=["nosplit", "split2"])
def test_conv_dgrad_classes_bn_bwd_partials(case, relu, cfg):
    """The BatchNorm-backward reductions fused into the data gradient -- sum g and sum g * xhat of
    the layer whose output gradient dx is -- against the column reduce of cilrs_bn_bwd on the
    stored dx."""
    L = _lib()
    lib = L.lib()
    N, H, W, Cin, Cout, splitk, with_scratch = case
    _, w, _, dy, _, add = _data(case)
    M = N * H * W
    g = torch.Generator().manual_seed(12)
    yb = (torch.randn(M, Cin, generator=g) * 1.3 + 0.2).cuda()     # raw input of the BatchNorm
    gamma = (torch.rand(Cin, generator=g) + 0.5).cuda()
    beta = (torch.rand(Cin, generator=g) - 0.5).cuda()
    rm, rv = torch.zeros(Cin, device="cuda"), torch.ones(Cin, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stats = torch.empty(4 * Cin, device="cuda")
    part = torch.full((lib.cilrs_bn_partial_floats(Cin),), float("nan"), device="cuda")
    z = torch.empty(M, Cin, device="cuda")
    L.check(lib.cilrs_bn_train_fwd(L.ptr(yb), M, Cin, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv),
                                   L.ptr(nbt), 0.1, 1e-5, None, relu, L.ptr(stats), L.ptr(part),
                                   L.ptr(z), stream()))
    dyd, wd, addd = nhwc(dy), ohwi(w), add.cuda()
    dx = torch.full((M, Cin), float("nan"), device="cuda")
    scratch = torch.empty(8 * dx.numel(), device="cuda") if with_scratch else None
    part.fill_(float("nan"))
    nblk = C.c_int(-1)
    L.check(lib.cilrs_conv2d_dgrad_bnbwd(L.ptr(dyd), L.ptr(wd), L.ptr(dx), L.ptr(addd), L.ptr(z),
                                         L.ptr(yb), L.ptr(stats), relu, L.ptr(part), C.byref(nblk),
                                         N, H, W, Cin, Cout, 3, 1, 1, cfg, splitk, L.ptr(scratch),
                                         scratch.numel() if with_scratch else 0, stream()))
    torch.cuda.synchronize()
    assert nblk.value > 0
    s1, s2 = _col_sums(part, nblk.value, Cin)
    assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
    dgamma, dbeta = torch.empty(Cin, device="cuda"), torch.empty(Cin, device="cuda")
    coef = torch.empty(3 * Cin, device="cuda")
    part2 = torch.empty(lib.cilrs_bn_partial_floats(Cin), device="cuda")
    dyo, gout = torch.empty(M, Cin, device="cuda"), torch.empty(M, Cin, device="cuda")
    L.check(lib.cilrs_bn_bwd(L.ptr(dx), L.ptr(z), L.ptr(yb), M, Cin, L.ptr(gamma), L.ptr(stats), relu,
                             L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), L.ptr(part2), L.ptr(dyo),
                             L.ptr(gout), stream()))
    torch.cuda.synchronize()
    gg = gout.double().cpu()                                      # g = dx * (z > 0), exact
    st = stats.double().cpu()
    xhat = (yb.double().cpu() - st[:Cin]) * st[Cin:2 * Cin]
    tol1 = M * _EPS * float(gg.abs().sum(0).max())
    # (each side also rounds xhat = (y - mean) * rstd in fp32: two more roundings per term and side)
    tol2 = (M + 4) * _EPS * float((gg * xhat).abs().sum(0).max())
    e1 = float((s1 - dbeta.double().cpu()).abs().max())
    e2 = float((s2 - dgamma.double().cpu()).abs().max())
    print(f"bn bwd partials {case} relu {relu} cfg {cfg}: nblk {nblk.value} sum g err {e1:.3e} "
          f"(tol {tol1:.3e}) sum g xhat err {e2:.3e} (tol {tol2:.3e})")
    assert e1 <= tol1 and e2 <= tol2
    # and against the float64 column sums of the stored g (xhat: two roundings, the product: one)
    x1 = float((s1 - gg.sum(0)).abs().max())
    x2 = float((s2 - (gg * xhat).sum(0)).abs().max())
    t1 = _ROWS * _EPS * float(gg.abs().sum(0).max())
    t2 = (_ROWS + 3) * _EPS * float((gg * xhat).abs().sum(0).max())
    print(f"  vs float64: sum g err {x1:.3e} (tol {t1:.3e}) sum g xhat err {x2:.3e} (tol {t2:.3e})")
    assert x1 <= t1 and x2 <= t2


# ---- which convolutions of a plan take classes ------------------------------------------------------
def _plan_classes(batch):
    L = _lib()
    lib = L.lib()
    net = C.c_void_p()
    L.check(lib.cilrs_net_create(batch, 88, 200, C.byref(net)))
    try:
        out = []
        conv = 0
        while True:
            numel, ch = C.c_size_t(), C.c_int()
            if lib.cilrs_net_activation_info(net, conv, None, None, C.byref(numel), C.byref(ch)) != 0:
                break
            f, d = C.c_int(-1), C.c_int(-1)
            L.check(lib.cilrs_net_conv_classes(net, conv, C.byref(f), C.byref(d)))
            out.append((conv, ch.value, numel.value // ch.value // batch, f.value, d.value))
            conv += 1
        return out
    finally:
        lib.cilrs_net_destroy(net)


def test_plan_takes_classes_for_layer4_only():
    """B = 128 at 88x200: the five 512 -> 512 3x3 / stride-1 convolutions of layer4 (3x7 maps), forward
    and data gradient, and nothing else; B = 1: nothing."""
    plan = _plan_classes(128)
    assert len(plan) == 36                       # ResNet-34: stem + 32 block convs + 3 down-samples
    taken = [(c, ch, px) for c, ch, px, f, d in plan if f or d]
    assert all(f == d for _, _, _, f, d in plan)
    assert len(taken) == 5, taken
    assert all(ch == 512 and px == 21 for _, ch, px in taken), taken
    # layer4.0.conv1 is the stride-2 256 -> 512 convolution, the down-sample is 1x1: neither
    assert sum(1 for _, ch, px, _, _ in plan if ch == 512 and px == 21) == 7
    assert not any(f or d for _, _, _, f, d in _plan_classes(1))
