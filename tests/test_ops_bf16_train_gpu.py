"""The bf16 training mode's operators where they differ from a plain convolution: fused epilogues
and the hand-off of column partials to BatchNorm, op by op through the C ABI, against float64.

  A. cilrs_conv2d_train_16 as a DATA GRADIENT on 16-bit tensors, both strides: the documented recipe
     (transposed, tap-flipped weights wT[ci][K-1-kh][K-1-kw][co]; stride 1: pad = K-1-pad_fwd;
     stride 2: up2 = 1, the parity-class launch) against autograd's input gradient of F.conv2d in
     double, as a bf16 result, with a bf16 addend, IN PLACE (addend16 == y16) and as an fp32 result.
  B. the BatchNorm-backward reductions that ride on those launches (bwd_partial): row count, extent,
     and the sums of g and g * xhat over the dx pixels, with z and y drawn so that the four parity
     classes differ visibly -- a class-to-pixel mix-up moves the sums by thousands of tolerances.
  C. the hand-off: conv2d_train_16(bn_partial / bwd_partial) -> bn16_train_fwd / bn16_bwd with
     pre_rows > 0, for 64-row tiles, 128-row persistent tiles and per-class tiles; and the fused
     path's UNPIVOTED variance (s2/M - mean^2) on channels with |mean|/std up to 2 R_net.
  D. the persistent 128-row kernel (conv16p_kernel) with every epilogue (0 plain, 1 addend, 2 bwd
     reductions, 3 both), its 3x3 / Cin >= 512 branch, and the fp16 instantiations (bf16 = 0).

Tolerances (none taken from the code under test):
  16-bit results   |got - ref| <= h |ref| + 1e-6 max|ref|, h = half a spacing of the format relative
                   to the value at most: 2^-8 (bf16), 2^-11 (fp16) -- one rounding of an fp32 sum
  fp32 results     5e-5 max|ref|
  column partials  summed over rows against float64 sums of WHAT THE KERNEL STORED: 1e-4 max(1, scale)
  BatchNorm        test_bn16_fwd_bwd_on_bf16_tensors' and test_bn_off_mean_within_the_networks_range's
Two 16-bit results that each meet h |ref| + t against the same reference are compared with each
other at twice that bound (triangle inequality; they may sit on either side of a rounding boundary).

Every output and partial buffer lies between guard bands (tests/_guards.py) and holds NaN before the
call; inputs are compared bit for bit afterwards.  References are computed once per case and shared.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from _guards import Inputs, all_finite, guarded
from test_ops_edges_gpu import EPS, HALF_BF16, R_NET_CEIL, _bn_params, _elementwise, ref_bn
from test_ops_gpu import conv16_train_rows as expect_rows    # the documented tile plan

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, F64, I16, I32 = torch.float32, torch.float64, torch.int16, torch.int32


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cdiv(a, b):
    return -(-a // b)


def _T(bf16):
    return torch.bfloat16 if bf16 else torch.float16


def _half(bf16):
    return 2.0 ** -8 if bf16 else 2.0 ** -11


def _bits(t):
    return t.contiguous().view(-1).view(I16 if t.element_size() == 2 else I32)


def _assert_close16(got, ref, bf16, what):
    """|got - ref| <= h |ref| + 1e-6 max|ref|"""
    err = (got - ref).abs()
    bound = _half(bf16) * ref.abs() + 1e-6 * float(ref.abs().max())
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst "
                                 f"error {float(err[bad].max()):.3e} at |ref| "
                                 f"{float(ref.abs()[bad][err[bad].argmax()]):.3e}")


def _assert_close32(got, ref, what):
    err, tol = float((got - ref).abs().max()), 5e-5 * float(ref.abs().max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _assert_colsums(part, rows, Cc, v1, v2, what):
    """part [2][Cc][rows] summed over rows against the float64 column sums of v1 / v2 [M][Cc]"""
    pp = part[:2 * Cc * rows].cpu().double().view(2, Cc, rows).sum(-1)
    for k, v in enumerate((v1, v2)):
        tol = 1e-4 * max(1.0, float(v.abs().sum(0).max()))
        err = float((pp[k] - v.sum(0)).abs().max())
        assert err <= tol, f"{what}: column sums [{k}] off by {err:.3e} > {tol:.3e}"


def classes(H, W, K, p):
    """The documented parity classes of a stride-2 data gradient over the dx grid [H][W]: class
    (ph, pw) = ((h + p) mod 2, (w + p) mod 2), in the order (0,0) (0,1) (1,0) (1,1), holds the pixels
    (2 i + h0, 2 j + w0), h0 = (ph - p) mod 2, and receives the taps kh = ph, ph + 2, ...  Returns
    (h0, w0, rows of the class grid, columns, taps) per class."""
    out = []
    for ph in (0, 1):
        for pw in (0, 1):
            h0, w0 = (ph - p) % 2, (pw - p) % 2
            out.append((h0, w0, len(range(h0, H, 2)), len(range(w0, W, 2)),
                        len(range(ph, K, 2)) * len(range(pw, K, 2))))
    return out


def class_rows(N, H, W, K, p, skip_untapped=False):
    """sum over the classes of cdiv(N Ho_c Wo_c, 64); in place (and without bwd_partial) the classes
    no tap reaches are not launched"""
    return sum(cdiv(N * hc * wc, 64) for _, _, hc, wc, nt in classes(H, W, K, p)
               if not (skip_untapped and nt == 0))


def train16(x, w, y16, y32, add, bnp, bz, by, bst, relu, bwp, geom, bf16):
    """cilrs_conv2d_train_16; geom = (N, H, W, Cin, Ho, Wo, Cout, K, stride, pad, up2); returns
    *partial_rows"""
    L = _L()
    rows = C.c_int(-1)
    L.check(L.lib().cilrs_conv2d_train_16(L.ptr(x), L.ptr(w), L.ptr(y16), L.ptr(y32), L.ptr(add),
                                          L.ptr(bnp), L.ptr(bz), L.ptr(by), L.ptr(bst), relu,
                                          L.ptr(bwp), *geom, bf16, C.byref(rows), stream()))
    torch.cuda.synchronize()
    return rows.value


# ---- A / B: the data gradient on 16-bit tensors ------------------------------------------------------
DGRAD_CASES = [
    # forward N, H, W, Cin, Cout, K, stride, pad
    (2, 12, 10, 64, 128, 3, 2, 1),       # even size
    (3, 7, 9, 64, 64, 3, 2, 1),          # odd size: the four classes have different sizes
    (2, 11, 13, 64, 256, 1, 2, 0),       # 1x1 stride 2, odd size: three classes no tap reaches
    (2, 12, 10, 64, 256, 1, 2, 0),       # 1x1 stride 2, even size
    (1, 1, 2, 64, 64, 3, 2, 1),          # classes with no pixel
    (1, 2, 1, 64, 64, 1, 2, 0),
    (3, 9, 14, 64, 64, 3, 1, 1),         # stride 1: pad = K-1-pad
    (2, 11, 13, 128, 64, 1, 1, 0),       # stride 1, 1x1
]
Y_OFFSET = (-3.0, -1.0, 1.0, 3.0)        # added to bwd_y16 per parity class
Z_OFFSET = (-1.5, -0.5, 0.5, 1.5)        # added to bwd_z16: 7 %, 31 %, 69 %, 93 % of z > 0


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


@functools.lru_cache(maxsize=None)
def dgrad_problem(case, bf16=1):
    """Operands (16-bit values on the CPU) and the float64 input gradient of one case, NHWC."""
    N, H, W, Cin, Cout, K, s, p = case
    T = _T(bf16)
    g = torch.Generator().manual_seed(100 + sum(case) + bf16)
    w16 = (torch.randn(Cout, Cin, K, K, generator=g) * (s / (K * K * Cout) ** 0.5)).to(T)
    x64 = torch.zeros(N, Cin, H, W, dtype=F64, requires_grad=True)
    y = F.conv2d(x64, w16.double(), None, s, p)
    Hof, Wof = y.shape[2], y.shape[3]
    dy16 = torch.randn(N, Cout, Hof, Wof, generator=g).to(T)
    dx = torch.autograd.grad(y, x64, dy16.double())[0].permute(0, 2, 3, 1).contiguous()
    add = torch.randn(N, H, W, Cin, generator=g).to(T)
    # the BatchNorm whose output gradient dx is: y / z with class-dependent statistics
    hh, ww = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    cls = (2 * ((hh + p) % 2) + (ww + p) % 2).view(1, H, W, 1)
    yoff, zoff = torch.tensor(Y_OFFSET)[cls], torch.tensor(Z_OFFSET)[cls]
    by = (torch.randn(N, H, W, Cin, generator=g) * 0.7 + yoff).to(T)
    bz = (torch.randn(N, H, W, Cin, generator=g) + zoff).to(T)
    bstats = torch.cat([torch.randn(Cin, generator=g) * 0.1, torch.rand(Cin, generator=g) + 0.5])
    reached = (((hh + p) % 2 < K) & ((ww + p) % 2 < K)).view(1, H, W, 1).expand(N, H, W, Cin)
    # documented layouts: gathered tensor = dy NHWC, weights = w.flip(2, 3).permute(1, 2, 3, 0)
    wT16 = w16.float().flip(2, 3).permute(1, 2, 3, 0).contiguous().to(T)
    geom = (N, Hof, Wof, Cout, H, W, Cin, K, s, p if s == 2 else K - 1 - p, 1 if s == 2 else 0)
    return dict(dx=dx, add=add, by=by, bz=bz, bstats=bstats, reached=reached, geom=geom,
                dy_nhwc=dy16.permute(0, 2, 3, 1).contiguous(), wT=wT16)


def bwd_sums(g, bz, by, bstats, relu):
    """float64 [M][C]: g masked by z > 0, and that times xhat = (y - mean) rstd"""
    Cc = g.shape[-1]
    gm = g.double().reshape(-1, Cc)
    if relu:
        gm = gm * (bz.double().reshape(-1, Cc) > 0)
    xh = (by.double().reshape(-1, Cc) - bstats[:Cc].double()) * bstats[Cc:].double()
    return gm, gm * xh


def class_swap_move(case, bf16=1):
    """What reading bwd_z16 / bwd_y16 at the pixel of the NEIGHBOURING class (w0 of the other column
    parity: column w ^ 1, kept inside the tensor) does to the two column sums, as multiples of their
    tolerances.  From the reference alone: g = the float64 gradient + addend, rounded to 16 bits."""
    P = dgrad_problem(case, bf16)
    W = case[2]
    g = (P["dx"] + P["add"].double()).to(_T(bf16))
    perm = (torch.arange(W) ^ 1).clamp_max(W - 1)
    a1, a2 = bwd_sums(g, P["bz"], P["by"], P["bstats"], 1)
    b1, b2 = bwd_sums(g, P["bz"][:, :, perm], P["by"][:, :, perm], P["bstats"], 1)
    return tuple(float((b.sum(0) - a.sum(0)).abs().max()) / (1e-4 * max(1.0, float(a.abs().sum(0).max())))
                 for a, b in ((a1, b1), (a2, b2)))


FORMS = ["bf16", "bf16+addend", "in-place", "fp32+addend"]


def run_dgrad_form(case, form, bf16):
    N, H, W, Cin, Cout, K, s, p = case
    P = dgrad_problem(case, bf16)
    T = _T(bf16)
    n = N * H * W * Cin
    xd, wd = P["dy_nhwc"].cuda(), P["wT"].cuda()
    addd = None if form == "bf16" else P["add"].cuda()
    if form == "fp32+addend":
        out, check = guarded(n, F32, NAN, 128 * Cin, f"dx32 {form}")
        y16, y32 = None, out
    else:
        out, check = guarded(n, T, NAN, 128 * Cin, f"dx16 {form}")
        y16, y32 = out, None
    if form == "in-place":
        out.copy_(addd.view(-1))
        addd = out
    inputs = Inputs(dy=xd, wT=wd, addend=None if form == "in-place" else addd)
    rows = train16(xd, wd, y16, y32, addd, None, None, None, None, 0, None, P["geom"], bf16)
    check()
    inputs.check()
    all_finite(out, f"dx {form}")
    got = out.cpu().double().view(N, H, W, Cin)
    want = P["dx"] if form == "bf16" else P["dx"] + P["add"].double()
    if form == "fp32+addend":
        _assert_close32(got, want, f"dx32 {case}")
    else:
        _assert_close16(got, want, bf16, f"dx16 {form} {case}")
    if s == 2:
        assert rows == class_rows(N, H, W, K, p, skip_untapped=form == "in-place"), rows
    else:
        exp = expect_rows(N * H * W, Cout, Cin, K)
        assert exp is None or rows == exp, (rows, exp)
    if s == 2 and K == 1:
        # pixels no tap reaches: the addend itself (in place: its bits untouched), zero without one
        un = ~P["reached"]
        assert bool(un.any()) and bool(P["reached"].any())
        assert float(P["dx"][un].abs().max()) == 0.0
        if form == "bf16":
            assert float(got[un].abs().max()) == 0.0
        elif form == "fp32+addend":
            assert torch.equal(got[un], P["add"].double()[un])
        else:
            gb = out.cpu().view(N, H, W, Cin).view(I16)
            assert torch.equal(gb[un], P["add"].view(I16)[un]), "unreached pixels do not hold the addend's bits"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_dgrad16_on_16bit_tensors(case, form):
    """A: cilrs_conv2d_train_16 given a real data-gradient problem in bf16 -- up2 = 1 (the parity-class
    launch) for the stride-2 cases, the stride-1 recipe pad = K-1-pad otherwise -- against autograd in
    double on the rounded operands.  Forms: bf16 result; + bf16 addend; the same in place
    (addend16 == y16: the classes no tap reaches are not launched and keep their bits); fp32 result +
    bf16 addend.  Every element of dx is written in the out-of-place forms (NaN before), nothing
    outside it; *partial_rows follows the documented class rule."""
    run_dgrad_form(case, form, 1)


FP16_CASES = [DGRAD_CASES[1], DGRAD_CASES[6]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", FP16_CASES, ids=_ids(FP16_CASES))
def test_dgrad16_fp16_instantiations(case, form):
    """The same with bf16 = 0 (conv_f16_kernel<_Float16, 64, 64, TRAIN>): one parity-class launch and
    one 64x64-family launch; bound 2^-11 |ref| + 1e-6 max|ref| (half an fp16 spacing)."""
    run_dgrad_form(case, form, 0)


def run_dgrad_bwd(case, form, relu, bf16=1):
    N, H, W, Cin, Cout, K, s, p = case
    P = dgrad_problem(case, bf16)
    T = _T(bf16)
    M = N * H * W
    xd, wd, addd = P["dy_nhwc"].cuda(), P["wT"].cuda(), P["add"].cuda()
    byd, bstd = P["by"].cuda(), P["bstats"].cuda()
    bzd = P["bz"].cuda() if relu else None
    rows_exp = class_rows(N, H, W, K, p) if s == 2 else cdiv(M, 64)      # (M < 512: 64-row tiles)
    out, check = guarded(M * Cin, T, NAN, 128 * Cin, f"dx16 {form}")
    part, check_part = guarded(2 * Cin * rows_exp, F32, NAN, 2 * Cin * rows_exp, "bwd_partial")
    if form == "in-place":
        out.copy_(addd.view(-1))
        addd = out
    inputs = Inputs(dy=xd, wT=wd, z=bzd, y=byd, stats=bstd, addend=None if form == "in-place" else addd)
    rows = train16(xd, wd, out, None, addd, None, bzd, byd, bstd, relu, part, P["geom"], bf16)
    check()
    check_part()
    inputs.check()
    assert rows == rows_exp, (rows, rows_exp)
    all_finite(out, "dx16")
    all_finite(part, "bwd_partial [2][C][rows]")
    got = out.cpu().view(N, H, W, Cin)
    _assert_close16(got.double(), P["dx"] + P["add"].double(), bf16, f"dx16 {form} {case}")
    v1, v2 = bwd_sums(got, P["bz"], P["by"], P["bstats"], relu)
    _assert_colsums(part, rows, Cin, v1, v2, f"bwd_partial {form} {case}")


@pytest.mark.parametrize("form", ["bf16+addend", "in-place"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_dgrad16_fused_bn_backward_reductions(case, form):
    """B: the same launches with bwd_partial / bwd_z16 / bwd_y16 / bwd_stats, bwd_relu = 1.
    *partial_rows = sum over the four classes of cdiv(N Ho_c Wo_c, 64) (computed here from the class
    rule; with bwd_partial every class is launched, in place too), exactly [2][C][rows] written, the
    row sums = float64 column sums of g and g xhat over ALL dx pixels, g = stored result * (z > 0).
    z and y carry a class-dependent offset (Z_OFFSET, Y_OFFSET), so the epilogue's map from row m of
    class (ph, pw) to pixel (2 i + h0, 2 j + w0) is visible in the sums: reading z / y at the
    neighbouring class's pixel moves sum g by 1.6e3 .. 8.0e3 tolerances and sum g xhat by 2.4e3 ..
    1.0e4 over the stride-2 cases with more than one column (class_swap_move, from the reference
    alone; asserted > 100)."""
    if case[6] == 2 and case[2] > 1:
        m1, m2 = class_swap_move(case)
        print(f"TRAIN16 class swap {case}: sum g moves {m1:.3g} tolerances, sum g xhat {m2:.3g}")
        assert m1 > 100 and m2 > 100
    run_dgrad_bwd(case, form, 1)


def test_dgrad16_fused_bn_backward_reductions_without_relu():
    """B with bwd_relu = 0 and bwd_z16 = NULL (the down-sample BatchNorm's reductions): g = the stored
    result, on a parity-class launch of odd size."""
    run_dgrad_bwd(DGRAD_CASES[1], "bf16+addend", 0)


# ---- C: the hand-off of column partials to BatchNorm ------------------------------------------------
def bn16_fwd(y16, M, Cc, gamma, beta, rm, rv, res, relu, part, pre_rows):
    """cilrs_bn16_train_fwd on device tensors; rm / rv are cloned.  Returns a dict of device outputs."""
    L = _L()
    stats, cs = guarded(4 * Cc, F32, NAN, 4 * Cc, "bn16 stats")
    z, cz = guarded(M * Cc, torch.bfloat16, NAN, 64 * Cc, "bn16 z16")
    rmd, rvd = rm.clone(), rv.clone()
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    L.check(L.lib().cilrs_bn16_train_fwd(L.ptr(y16), M, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(rmd),
                                         L.ptr(rvd), L.ptr(nbt), 0.1, EPS, L.ptr(res), relu,
                                         L.ptr(stats), L.ptr(part), L.ptr(z), pre_rows, stream()))
    cs()
    cz()
    assert int(nbt) == 1
    all_finite(stats, "bn16 stats")
    all_finite(z, "bn16 z16")
    return dict(stats=stats, z=z.view(M, Cc), rm=rmd, rv=rvd)


def bn16_bwd(dz16, z16, y16, M, Cc, gamma, stats, relu, part, pre_rows):
    L = _L()
    dy, c1 = guarded(M * Cc, torch.bfloat16, NAN, 64 * Cc, "bn16 dy16")
    gout, c2 = guarded(M * Cc, torch.bfloat16, NAN, 64 * Cc, "bn16 g_out16")
    dgam, c3 = guarded(Cc, F32, NAN, Cc, "bn16 dgamma")
    dbet, c4 = guarded(Cc, F32, NAN, Cc, "bn16 dbeta")
    coef, c5 = guarded(3 * Cc, F32, NAN, 3 * Cc, "bn16 coef3c")
    L.check(L.lib().cilrs_bn16_bwd(L.ptr(dz16), L.ptr(z16), L.ptr(y16), M, Cc, L.ptr(gamma),
                                   L.ptr(stats), relu, L.ptr(dgam), L.ptr(dbet), L.ptr(coef),
                                   L.ptr(part), L.ptr(dy), L.ptr(gout), pre_rows, stream()))
    for c in (c1, c2, c3, c4, c5):
        c()
    for t, name in ((dy, "dy16"), (gout, "g_out16"), (dgam, "dgamma"), (dbet, "dbeta"), (coef, "coef3c")):
        all_finite(t, "bn16 " + name)
    return dict(dy=dy.view(M, Cc), gout=gout.view(M, Cc), dgamma=dgam, dbeta=dbet, coef=coef)


def bn_partial_buffer(Cc, name):
    """cilrs_bn_partial_floats(C) floats of NaN between guards: what a convolution epilogue fills with
    [2][C][rows] and BatchNorm then reads with pre_rows = rows"""
    n = _L().lib().cilrs_bn_partial_floats(Cc)
    return guarded(n, F32, NAN, 2 * Cc * 128, name)


def assert_partial_extent(part, check, Cc, rows, name):
    check()
    all_finite(part[:2 * Cc * rows], name + " [2][C][rows]")
    assert bool(torch.isnan(part[2 * Cc * rows:]).all()), name + ": written past [2][C][rows]"


# one launch per tile family; (name, forward-style case, as a stride-2 data gradient?)
HANDOFF = [
    ("64-row tiles", (3, 9, 14, 64, 128, 3, 1, 1), False),
    ("128-row persistent tiles", (13, 25, 25, 64, 512, 1, 1, 0), False),
    ("parity classes", (3, 7, 9, 64, 64, 3, 2, 1), True),
]
HANDOFF_IDS = [h[0].replace(" ", "-") for h in HANDOFF]


@functools.lru_cache(maxsize=None)
def handoff_problem(name):
    """A launch whose output channels have means well away from zero, as the network's BatchNorm
    inputs do: gathered tensor x = relu(randn) (mean 0.4), and every output channel's weights sum to
    +-(1 .. 3).  Forward-style launches enumerate the convolution's output, the parity-class launch
    the dx grid of the stride-2 case.  Returns CPU operands and the launch geometry."""
    _, case, as_dgrad = next(h for h in HANDOFF if h[0] == name)
    N, H, W, Cin, Cout, K, s, p = case
    g = torch.Generator().manual_seed(500 + sum(case))
    if as_dgrad:            # gathered = dy [N][Hof][Wof][Cout], enumerated = dx [N][H][W][Cin]
        Hof, Wof = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        gin, gout, gh, gw, oh, ow = Cout, Cin, Hof, Wof, H, W
        geom = (N, Hof, Wof, Cout, H, W, Cin, K, 2, p, 1)
    else:
        oh, ow = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        gin, gout, gh, gw = Cin, Cout, H, W
        geom = (N, H, W, Cin, oh, ow, Cout, K, s, p, 0)
    x = torch.relu(torch.randn(N, gh, gw, gin, generator=g)).to(torch.bfloat16)
    w = torch.randn(gout, K, K, gin, generator=g) / (K * K * gin) ** 0.5
    target = (1 + 2 * torch.rand(gout, generator=g)) * torch.where(torch.rand(gout, generator=g) < 0.5, -1.0, 1.0)
    w = (w + ((target - w.sum((1, 2, 3))) / (K * K * gin)).view(-1, 1, 1, 1)).to(torch.bfloat16)
    M = N * oh * ow
    return dict(x=x, w=w, geom=geom, M=M, C=gout, K=K, Cin=gin, up2=as_dgrad, case=case,
                rows=class_rows(N, H, W, K, p) if as_dgrad else None)


def handoff_rows(P):
    return P["rows"] if P["up2"] else expect_rows(P["M"], P["Cin"], P["C"], P["K"])


@pytest.mark.parametrize("name", [h[0] for h in HANDOFF], ids=HANDOFF_IDS)
def test_handoff_conv_epilogue_to_bn16_forward(name):
    """C.1: conv2d_train_16(bn_partial) -> bn16_train_fwd(pre_rows = rows) for each tile family (the
    persistent one only where the plan picks it: 256 compute units).  The fused call must meet the
    tolerances of test_bn16_fwd_bwd_on_bf16_tensors against float64 BatchNorm of the STORED y16 (z:
    2^-8 |ref| + 1e-5, running statistics 1e-5), as the unfused call (pre_rows = 0) on the same y16
    does; mean within 1e-5 relative and rstd within 1e-4 relative of the unfused call's; the partial
    buffer is only read.  Channel means are 0.1 .. 1.2 in magnitude (asserted > 0.02 on the
    reference), so 'relative' is meaningful."""
    P = handoff_problem(name)
    M, Cc = P["M"], P["C"]
    xd, wd = P["x"].cuda(), P["w"].cuda()
    y16, cy = guarded(M * Cc, torch.bfloat16, NAN, 128 * Cc, "y16")
    part, cp = bn_partial_buffer(Cc, "bn_partial")
    rows = train16(xd, wd, y16, None, None, part, None, None, None, 0, None, P["geom"], 1)
    cy()
    all_finite(y16, "y16")
    exp = handoff_rows(P)
    assert exp is None or rows == exp, (rows, exp)
    assert_partial_extent(part, cp, Cc, rows, "bn_partial")
    ys = y16.cpu().view(M, Cc)
    _assert_colsums(part, rows, Cc, ys.double(), ys.double() ** 2, f"bn_partial {name}")
    g = torch.Generator().manual_seed(77)
    gamma, beta, rm, rv = _bn_params(Cc, g)
    res = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    ref = ref_bn(ys, gamma, beta, rm, rv, res, 1, torch.zeros(M, Cc))
    mean64 = ys.double().mean(0)
    assert float(mean64.abs().min()) > 0.02
    dev = [t.cuda() for t in (gamma, beta, rm, rv, res)]
    before = _bits(part).clone()
    fused = bn16_fwd(y16, M, Cc, *dev, 1, part, rows)
    cp()
    assert torch.equal(_bits(part), before), "bn16_train_fwd(pre_rows > 0) wrote the partial buffer"
    spare, cs = bn_partial_buffer(Cc, "bn16 partial (unfused)")
    plain = bn16_fwd(y16, M, Cc, *dev, 1, spare, 0)
    cs()
    zref = ref["z"]
    for tag, got in (("fused", fused), ("unfused", plain)):
        ez = (got["z"].cpu().double() - zref).abs()
        assert bool((ez <= HALF_BF16 * zref.abs() + 1e-5).all()), (tag, float(ez.max()))
        assert float((got["rm"].cpu().double() - ref["rm"]).abs().max()) <= 1e-5, tag
        assert float((got["rv"].cpu().double() - ref["rv"]).abs().max()) <= 1e-5, tag
    ez = (fused["z"].cpu().double() - plain["z"].cpu().double()).abs()
    assert bool((ez <= 2 * (HALF_BF16 * zref.abs() + 1e-5)).all())
    sf, sp = fused["stats"].cpu().double(), plain["stats"].cpu().double()
    emean = float(((sf[:Cc] - sp[:Cc]).abs() / sp[:Cc].abs()).max())
    erstd = float(((sf[Cc:2 * Cc] - sp[Cc:2 * Cc]).abs() / sp[Cc:2 * Cc]).max())
    print(f"TRAIN16 hand-off fwd {name}: rows {rows}, mean rel {emean:.2e}, rstd rel {erstd:.2e}")
    assert emean <= 1e-5 and erstd <= 1e-4
    assert float(((sp[:Cc] - mean64).abs() / mean64.abs()).max()) <= 1e-5


@pytest.mark.parametrize("name", [h[0] for h in HANDOFF], ids=HANDOFF_IDS)
def test_handoff_conv_epilogue_to_bn16_backward(name):
    """C.2: a BatchNorm layer (y16, its own z16 and stats from bn16_train_fwd, residual + ReLU), the
    gradient of its output produced by conv2d_train_16(+ addend, bwd_partial), then
    bn16_bwd(pre_rows = rows) on that stored gradient.  dgamma / dbeta (1e-4 max(1, |ref|)), dy16
    (2^-8 |ref| + 1e-5 max|ref|) and g_out16 (exact under the kernel's mask) against float64, and
    against bn16_bwd(pre_rows = 0) on the same tensors."""
    P = handoff_problem(name)
    M, Cc = P["M"], P["C"]
    g = torch.Generator().manual_seed(91)
    y = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    res = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    add = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    gamma, beta, rm, rv = _bn_params(Cc, g)
    yd, resd, addd, gd = y.cuda(), res.cuda(), add.cuda(), gamma.cuda()
    spare, _ = bn_partial_buffer(Cc, "bn16 partial")
    layer = bn16_fwd(yd, M, Cc, gd, beta.cuda(), rm.cuda(), rv.cuda(), resd, 1, spare, 0)
    z16, stats = layer["z"], layer["stats"]
    xd, wd = P["x"].cuda(), P["w"].cuda()
    dz16, cd = guarded(M * Cc, torch.bfloat16, NAN, 128 * Cc, "dz16")
    part, cp = bn_partial_buffer(Cc, "bwd_partial")
    inputs = Inputs(x=xd, w=wd, z=z16, y=yd, stats=stats, addend=addd)
    rows = train16(xd, wd, dz16, None, addd, None, z16, yd, stats, 1, part, P["geom"], 1)
    cd()
    inputs.check()
    all_finite(dz16, "dz16")
    exp = handoff_rows(P)
    assert exp is None or rows == exp, (rows, exp)
    assert_partial_extent(part, cp, Cc, rows, "bwd_partial")
    before = _bits(part).clone()
    fused = bn16_bwd(dz16, z16, yd, M, Cc, gd, stats, 1, part, rows)
    cp()
    assert torch.equal(_bits(part), before), "bn16_bwd(pre_rows > 0) wrote the partial buffer"
    plain = bn16_bwd(dz16, z16, yd, M, Cc, gd, stats, 1, spare, 0)
    # float64 BatchNorm backward of the stored gradient under the kernel's own mask
    dzs, zk, y64 = dz16.cpu().view(M, Cc).double(), z16.cpu().double(), y.double()
    gm = dzs * (zk > 0)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (y64 - mean) * rstd
    dbeta, dgamma = gm.sum(0), (gm * xh).sum(0)
    dy = gamma.double() * rstd * (gm - dbeta / M - xh * dgamma / M)
    tg, tb = 1e-4 * max(1.0, float(dgamma.abs().max())), 1e-4 * max(1.0, float(dbeta.abs().max()))
    bound = HALF_BF16 * dy.abs() + 1e-5 * float(dy.abs().max())
    for tag, got in (("fused", fused), ("unfused", plain)):
        assert torch.equal(got["gout"].cpu().double(), gm), tag
        assert float((got["dgamma"].cpu().double() - dgamma).abs().max()) <= tg, tag
        assert float((got["dbeta"].cpu().double() - dbeta).abs().max()) <= tb, tag
        edy = (got["dy"].cpu().double() - dy).abs()
        assert bool((edy <= bound).all()), (tag, float((edy / bound).max()))
    assert torch.equal(_bits(fused["gout"]), _bits(plain["gout"]))
    assert float((fused["dgamma"] - plain["dgamma"]).abs().max()) <= tg
    assert float((fused["dbeta"] - plain["dbeta"]).abs().max()) <= tb
    assert bool(((fused["dy"].cpu().double() - plain["dy"].cpu().double()).abs() <= 2 * bound).all())
    print(f"TRAIN16 hand-off bwd {name}: rows {rows}, dgamma err "
          f"{float((fused['dgamma'].cpu().double() - dgamma).abs().max()):.2e} (tol {tg:.2e})")


@pytest.mark.parametrize("M", [3300, 21, 65500])
@pytest.mark.parametrize("sigma", [1.0, 0.05])
@pytest.mark.parametrize("r", [0, R_NET_CEIL, 2 * R_NET_CEIL])
def test_handoff_off_mean_channels_on_the_unpivoted_path(r, sigma, M):
    """C.3: with pre_rows > 0 the finalise takes var = s2/M - mean^2 from sums of y and y*y themselves
    (no pivot).  y16 = randn sigma + r sigma (+-1 per channel), |mean|/std = r up to twice the
    network's largest (R_net = 5.20, oracle/bn_input_ratio.py), goes through a 1x1 convolution with
    the identity as weights, which stores y16 bit for bit and hands its tile partials (64-row tiles;
    128-row persistent tiles at M = 65500 on 256 compute units) to bn16_train_fwd; the backward is
    fused the same way (identity convolution of dz16 with bwd_partial, bwd_relu = 0 -> bn16_bwd with
    pre_rows).  The parity tolerances of test_bn_off_mean_within_the_networks_range, unchanged.
    They hold.  Measured on MI355X, largest error as a fraction of its bound over the 18 cases:
    dgamma 0.009, dbeta 0.001, running_mean 0.063, running_var 0.008.  z and dy sit at 0.88 .. 0.99
    of theirs at every r, r = 0 included, as any correctly rounded bf16 tensor does (the bound's
    relative term IS half a bf16 spacing); the statistics behind them are printed on their own: mean
    within 9.3e-7 of a std, rstd within 3.0e-7 relative (r = 12 / r = 6, M = 65500), together under
    4e-6 on z -- a fifth of the absolute part of its bound.  (The squares of bf16 values are exact in
    fp32, so the sum of squares rounds only where partial sums are added.)"""
    Cc = 64
    g = torch.Generator().manual_seed(1000 * r + M + int(100 * sigma))
    sign = torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
    y = (torch.randn(M, Cc, generator=g) * sigma + r * sigma * sign).to(torch.bfloat16)
    dz = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    gamma, beta, rm, rv = _bn_params(Cc, g)
    ref = ref_bn(y, gamma, beta, rm, rv, None, 0, dz)
    eye = torch.eye(Cc).to(torch.bfloat16).view(Cc, 1, 1, Cc).cuda()
    geom = (1, M, 1, Cc, M, 1, Cc, 1, 1, 0, 0)
    yd, dzd, gd = y.cuda(), dz.cuda(), gamma.cuda()
    # forward: identity convolution -> tile partials -> BatchNorm
    y16, cy = guarded(M * Cc, torch.bfloat16, NAN, 128 * Cc, "y16")
    part, cp = bn_partial_buffer(Cc, "bn_partial")
    rows = train16(yd, eye, y16, None, None, part, None, None, None, 0, None, geom, 1)
    cy()
    assert torch.equal(_bits(y16), _bits(yd)), "the identity convolution did not reproduce y16"
    exp = expect_rows(M, Cc, Cc, 1)
    assert exp is None or rows == exp, (rows, exp)
    assert_partial_extent(part, cp, Cc, rows, "bn_partial")
    fwd = bn16_fwd(y16, M, Cc, gd, beta.cuda(), rm.cuda(), rv.cuda(), None, 0, part, rows)
    # backward: identity convolution of dz with the mask-free reductions -> BatchNorm backward
    d16, cd = guarded(M * Cc, torch.bfloat16, NAN, 128 * Cc, "dz16")
    bpart, cb = bn_partial_buffer(Cc, "bwd_partial")
    brows = train16(dzd, eye, d16, None, None, None, None, y16, fwd["stats"], 0, bpart, geom, 1)
    cd()
    assert torch.equal(_bits(d16), _bits(dzd))
    assert brows == expect_rows(M, Cc, Cc, 1, masked=False), brows
    assert_partial_extent(bpart, cb, Cc, brows, "bwd_partial")
    bwd = bn16_bwd(d16, None, y16, M, Cc, gd, fwd["stats"], 0, bpart, brows)
    assert torch.equal(_bits(bwd["gout"]), _bits(dzd))
    got = {"z": fwd["z"], "dy": bwd["dy"], "dgamma": bwd["dgamma"], "dbeta": bwd["dbeta"],
           "rm": fwd["rm"], "rv": fwd["rv"]}
    got = {k: v.cpu().double() for k, v in got.items()}
    _, fz = _elementwise(got["z"], ref["z"], 2e-5 * max(1.0, float(ref["z"].abs().max())), HALF_BF16)
    _, fdy = _elementwise(got["dy"], ref["dy"], 5e-5 * max(1.0, float(ref["dy"].abs().max())), HALF_BF16)
    fg = float((got["dgamma"] - ref["dgamma"]).abs().max()) / (5e-5 * max(1.0, float(ref["dgamma"].abs().max())))
    fb = float((got["dbeta"] - ref["dbeta"]).abs().max()) / (5e-5 * max(1.0, float(ref["dbeta"].abs().max())))
    frm = float(((got["rm"] - ref["rm"]).abs() / ref["rm"].abs().clamp_min(1.0)).max()) / 1e-6
    frv = float(((got["rv"] - ref["rv"]).abs() / ref["rv"].abs().clamp_min(1.0)).max()) / 1e-5
    # the statistics themselves, before any bf16 rounding: mean in units of the channel's std, rstd relative
    y64 = y.double()
    mean64, rstd64 = y64.mean(0), 1.0 / torch.sqrt(y64.var(0, unbiased=False) + EPS)
    st = fwd["stats"].cpu().double()
    emean = float(((st[:Cc] - mean64).abs() * rstd64).max())
    erstd = float((st[Cc:2 * Cc] / rstd64 - 1.0).abs().max())
    print(f"TRAIN16 off-mean fused M={M} sigma={sigma} r={r} rows={rows}: fractions of the bounds "
          f"z {fz:.3f} dy {fdy:.3f} dgamma {fg:.3f} dbeta {fb:.3f} rm {frm:.3f} rv {frv:.3f}; "
          f"mean err / std {emean:.2e}, rstd rel err {erstd:.2e}")
    assert fz <= 1.0 and fdy <= 1.0
    assert fg <= 1.0 and fb <= 1.0
    assert frm <= 1.0 and frv <= 1.0


# ---- D: the persistent 128-row family, every epilogue ---------------------------------------------------
PERSIST_1X1 = (13, 25, 25, 64, 512, 1, 1, 0)       # M = 8125: 64 tiles of 128 rows, the last one 61
PERSIST_3X3 = (9, 21, 21, 512, 1024, 3, 1, 1)      # M = 3969: 32 tiles, the last one ONE row


@functools.lru_cache(maxsize=None)
def forward_problem(case, bf16, f64):
    N, H, W, Cin, Cout, K, s, p = case
    T = _T(bf16)
    g = torch.Generator().manual_seed(300 + sum(case) + bf16)
    x = torch.randn(N, Cin, H, W, generator=g).to(T)
    w = (torch.randn(Cout, Cin, K, K, generator=g) / (K * K * Cin) ** 0.5).to(T)
    if f64:
        ref = F.conv2d(x.double(), w.double(), None, s, p)
    else:
        torch.set_num_threads(16)
        ref = F.conv2d(x.float(), w.float(), None, s, p).double()
    Ho, Wo = ref.shape[2], ref.shape[3]
    M = N * Ho * Wo
    ref = ref.permute(0, 2, 3, 1).reshape(M, Cout)
    add = torch.randn(M, Cout, generator=g).to(T)
    bz = torch.randn(M, Cout, generator=g).to(T)
    by = torch.randn(M, Cout, generator=g).to(T)
    bstats = torch.cat([torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5])
    return dict(ref=ref, add=add, bz=bz, by=by, bstats=bstats, M=M,
                x=x.permute(0, 2, 3, 1).contiguous(), w=w.permute(0, 2, 3, 1).contiguous(),
                geom=(N, H, W, Cin, Ho, Wo, Cout, K, s, p, 0))


def run_forward_epilogue(case, epi, bf16, f64=True):
    """one launch of the forward form with epilogue bits: 1 = 16-bit addend, 2 = BatchNorm-backward
    reductions (ReLU mask); epilogue 0 carries the forward's bn_partial"""
    P = forward_problem(case, bf16, f64)
    T = _T(bf16)
    M, Cin, Cout, K = P["M"], case[3], case[4], case[5]
    xd, wd = P["x"].cuda(), P["w"].cuda()
    addd = P["add"].cuda() if epi & 1 else None
    bzd, byd, bstd = (P["bz"].cuda(), P["by"].cuda(), P["bstats"].cuda()) if epi & 2 else (None,) * 3
    y16, cy = guarded(M * Cout, T, NAN, 128 * Cout, f"y16 epilogue {epi}")
    nmax = 2 * Cout * cdiv(M, 64)
    part, cp = guarded(nmax, F32, NAN, nmax, "column partials")
    inputs = Inputs(x=xd, w=wd, addend=addd, z=bzd, y=byd, stats=bstd)
    rows = train16(xd, wd, y16, None, addd, part if epi == 0 else None, bzd, byd, bstd, 1 if epi & 2 else 0,
                   part if epi & 2 else None, P["geom"], bf16)
    cy()
    inputs.check()
    all_finite(y16, "y16")
    exp = expect_rows(M, Cin, Cout, K)
    assert exp is None or rows == exp, f"epilogue {epi}: {rows} partial rows, the plan's family has {exp}"
    got = y16.cpu().view(M, Cout)
    want = P["ref"] + (P["add"].double() if epi & 1 else 0.0)
    _assert_close16(got.double(), want, bf16, f"y16 epilogue {epi} {case}")
    if epi == 0 or epi & 2:
        assert_partial_extent(part, cp, Cout, rows, "column partials")
        if epi == 0:
            v1, v2 = got.double(), got.double() ** 2
        else:
            v1, v2 = bwd_sums(got, P["bz"], P["by"], P["bstats"], 1)
        _assert_colsums(part, rows, Cout, v1, v2, f"partials epilogue {epi} {case}")
    if epi == 1:        # the fp32 result of the same launch (the gradient handed to the fp32 stem)
        y32, c32 = guarded(M * Cout, F32, NAN, 128 * Cout, "y32")
        r32 = train16(xd, wd, None, y32, addd, None, None, None, None, 0, None, P["geom"], bf16)
        c32()
        inputs.check()
        assert exp is None or r32 == exp
        _assert_close32(y32.cpu().double().view(M, Cout), want, f"y32 epilogue 1 {case}")


@pytest.mark.parametrize("epi,bf16", [(0, 1), (1, 1), (2, 1), (3, 1), (0, 0)],
                         ids=["plain", "addend", "bwd", "addend+bwd", "plain-fp16"])
def test_conv16_persistent_family_every_epilogue(epi, bf16):
    """D: the smallest 1x1 launch the plan gives to conv16p_kernel on 256 compute units
    (cdiv(M,128) * Cout/64 = 512 tiles; M = 8125 leaves a last tile of 61 rows) with each of its four
    compile-time epilogues, and epilogue 0 in fp16.  Against F.conv2d in double of the rounded
    operands; partials against sums of the stored result; *partial_rows == cdiv(M, 128) says the
    128-row family ran (asserted on a 256-CU device only)."""
    run_forward_epilogue(PERSIST_1X1, epi, bf16)


def test_conv16_persistent_family_3x3_wide_reduction():
    """D: the 3x3 branch of the plan (Cin >= 512) at the smallest M that reaches it with Cout = 1024
    (32 x 16 = 512 tiles; M = 3969, a last tile of one row): 72 K-tiles per tile, forward form +
    addend (epilogue 1), bf16 and fp32 results.  Reference: torch's fp32 CPU convolution."""
    run_forward_epilogue(PERSIST_3X3, 1, 1, f64=False)
