"""Every op-level entry point of the C-ABI called once per case with

  * every output and every scratch buffer inside guard bands (tests/_guards.py),
  * every scratch buffer sized exactly as the library's own size function reports,
  * outputs pre-filled with NaN,

and afterwards: (a) all guards bit-identical to their pattern, (b) all `const` inputs unchanged,
(c) the output finite wherever the header says every element is written.  No CPU reference: parity
is test_ops_gpu.py's / test_infer16_gpu.py's business, whose case lists are imported, not copied.

Guard lengths: 128 rows x the row pitch for convolution and linear outputs (the tallest tile any of
these kernels stores), one whole array for BatchNorm partials, the buffer's own length for small
vectors; never less than 4096 bytes.

Which case exercises an entry's ragged tail / its plan at the benchmark batch (N = 128):

  conv2d_fwd, conv2d_dgrad     (1, 3, 7, 512, 512, 3, 1, 1): M = 21 rows under 64- and 128-row tiles,
                               every forced tile and split-K / TRUNK_SHAPES at N = 128, auto plan;
                               each with scratch capacity 0 (NULL), one slab, the plan's 36 M floats
  conv2d_wgrad                 the same M = 21 case / (128,) + TRUNK_SHAPES (K-slabs over grid.z)
  the three above, Bottleneck  BOTTLENECK_GUARD_CASES: (1, 3, 7, 2048, 512, 1, 1, 0), M = 21 under the
                               longest 1x1 K loop; (7, 3, 7, 512, 2048, 1, 1, 0) and (5, 6, 13, 1024,
                               2048, 1, 2, 0), the widest rows; (2, 22, 50, 64, 64, 1, 1, 0), the shortest
                               K loop and a one-tile weight gradient / none
  conv2d_fwd_stats, conv2d_dgrad_bnbwd   the same four (the data-gradient form: the stride-1 ones), a
                               128-row tile, the 64-row tile, the automatic plan and two forced slabs,
                               partial buffer of exactly bn_partial_floats / none
  stem_conv_fwd, _wgrad        (9, 86, 199) and (2, 26, 400): partial last tiles / (128, 88, 200)
  stem_conv_dgrad              (1, 37, 51), (9, 86, 199), pitched rows / (128, 88, 200)
  conv2d_wino_fwd, _pre, _split, _fold_fwd, _dgrad, _wgrad, wino_filter_transform
                               (1, 5, 3, 8, 64): fewer tiles than a block (forward forms) and
                               (3, 11, 25, 128, 128): half-filled edge tiles / the two N = 128 cases
  conv2d_fwd_16, _dgrad_16, _wgrad_16   (5, 7, 7, 64, 64, 3, 2, 1), (3, 5, 9, 256, 128, 1, 1, 0) / none
                               (the fp32-in entries have no batch plan of their own)
  conv2d_train_16              (33, 44, 50, 256, 128, 1, 1, 0): M % 128 = 24 / (64, 44, 100, ...)
  conv2d_infer_16              RAGGED_CASES: M = 6, 63, 65, 127, 129 / (64, 22, 50, ...) serving size
  stem_infer_16, maxpool_infer_16, avgpool_infer_16   (3, 9, 253), (1, 7, 9), HW = 21 / none
  bn_train_fwd, bn_bwd, bn_eval_fwd, bn_bwd_frozen     M = 1, 21, 63, 65 / M = 35,200 (128 x 11 x 25)
  bn16_train_fwd, bn16_bwd     M = 1, 63, 65, 77 / M = 70,400
  maxpool_fwd, _bwd, bn_bwd_pool_frozen   (1, 7, 9), (1, 19, 26) / none
  linear_fwd, linear_bwd       (70, 100, 45), (7, 256, 1), (128, 1, 128) / batch 128 rows
  dropout, loss, eval_accumulate   (5, 3, 7) / B = 257, 300: a second trip of the 256-thread loop
  grad_sqnorm, adam_step, adam_step_groups, scale   n = 4 / n = 4 (4096 x 256 + 3): a second
                               grid-stride trip with a ragged end
  saliency_map, augment_u8, batch_assemble   the smallest shapes of their own test files
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from _guards import Inputs, all_finite, guarded, guarded_rows
from test_infer16_gpu import BOTTLENECK_CASES, RAGGED_CASES
from test_ops_bottleneck_gpu import BOTTLENECK_F32_CASES, STATS_PLANS
from test_ops_gpu import (CONV16_CASES, CONV16T_CASES, CONV_CASES, LINEAR_CASES,
                          PLAN_KSPLIT_FLOATS, TRUNK_SHAPES, WINO_CASES)

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16, F16, U8, I16, I64, F64 = (torch.float32, torch.bfloat16, torch.float16, torch.uint8,
                                     torch.int16, torch.int64, torch.float64)


SCRATCH_GUARD_CAP = 8 << 20        # elements: the guard after a scratch buffer is as long as the
#                                    buffer itself up to this (the plan's 36 M-float split-K scratch)


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(20)


def R(*shape, dtype=F32, scale=1.0):
    """a const input, drawn on the device (no reference needs its values on the host)"""
    return (torch.randn(*shape, device="cuda") * scale).to(dtype)


class Guards:
    """the guarded buffers and the input snapshot of one call"""

    def __init__(self):
        self.checks, self.finite, self.inputs = [], [], None

    def buf(self, shape, dtype=F32, fill=NAN, guard=0, name="out", finite=True):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        v, chk = guarded(n, dtype, fill, max(guard, 0), name)
        self.checks.append(chk)
        v = v.view(shape)
        if finite and dtype.is_floating_point and fill is not None and fill != fill:
            self.finite.append((name, v))
        return v

    def scratch(self, numel, dtype=F32, name="scratch"):
        """exactly `numel` elements; NaN (all-ones for integer types) so that a read of something the
        call did not write first shows up in the outputs"""
        fill = NAN if dtype.is_floating_point else (255 if dtype == U8 else -1)
        return self.buf(int(numel), dtype, fill, min(int(numel), SCRATCH_GUARD_CAP), name, finite=False)

    def rows(self, rows, cols, ld, dtype=F32, fill=NAN, guard=0, name="matrix"):
        full, logical, chk = guarded_rows(rows, cols, ld, dtype, fill, guard, name)
        self.checks.append(chk)
        if fill != fill:
            self.finite.append((name, logical))
        return full, logical

    def const(self, **tensors):
        self.inputs = Inputs(**tensors)

    def verify(self):
        torch.cuda.synchronize()
        for chk in self.checks:
            chk()
        if self.inputs is not None:
            self.inputs.check()
        for name, v in self.finite:
            all_finite(v, name)


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---- the helper itself ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, U8, F64])
def test_guards_notice_a_store_on_either_side_and_in_a_pad_column(dtype):
    """a store one element outside the view on either side, a store into a pad column and a store
    into a const input are each reported (plain torch stores inside the helper's own allocation)"""
    for off in (-1, 0):
        view, check = guarded(100, dtype, 0, name="probe")
        check()
        base = view.untyped_storage()
        flat = torch.empty(0, dtype=dtype, device="cuda").set_(base)
        at = view.storage_offset() + (off if off < 0 else view.numel())
        flat[at] = 1
        with pytest.raises(AssertionError, match="probe: written (before its start|past its end)"):
            check()
    full, logical, check = guarded_rows(5, 3, 7, F32, 0.0, name="probe rows")
    logical.fill_(2.0)
    check()
    full[3, 4] = 2.0
    with pytest.raises(AssertionError, match="pad columns written, first in row 3"):
        check()
    x = torch.ones(8, device="cuda")
    snap = Inputs(x=x)
    snap.check()
    x[5] = -1.0
    with pytest.raises(AssertionError, match="const input `x` was modified"):
        snap.check()


# ---- fp32 implicit GEMM: forward and data gradient -------------------------------------------------
FWD_PLANS = [(-1, 0), (0, 1), (1, 1), (2, 1), (1, 3), (2, 2), (3, 1), (4, 1), (5, 1), (5, 2), (4, 3)]
DGRAD_PLANS = [(-1, 0), (1, 1), (2, 2), (4, 1), (5, 2), (5, 1)]
CAPACITIES = ["none", "one_slab", "plan"]
# the ragged and the widest of the ResNet-50 variant's shapes
BOTTLENECK_GUARD_CASES = [(1, 3, 7, 2048, 512, 1, 1, 0), (7, 3, 7, 512, 2048, 1, 1, 0),
                          (5, 6, 13, 1024, 2048, 1, 2, 0), (2, 22, 50, 64, 64, 1, 1, 0)]
assert set(BOTTLENECK_GUARD_CASES) <= set(BOTTLENECK_F32_CASES)
FWD_CASES = [(c, cfg, sk) for c in CONV_CASES + BOTTLENECK_GUARD_CASES for cfg, sk in FWD_PLANS
             if not (cfg in (0, 3) and c[4] % 128)]          # the 128-wide tile needs Cout % 128 == 0
DGRAD_CASES = [(c, cfg, sk) for c in CONV_CASES + BOTTLENECK_GUARD_CASES for cfg, sk in DGRAD_PLANS]


def _capacity(g, kind, out_numel):
    """(scratch tensor or None, stated capacity): the guard sits right after the stated capacity"""
    if kind == "none":
        return None, 0
    n = out_numel if kind == "one_slab" else PLAN_KSPLIT_FLOATS
    return g.scratch(n, name=f"split-K scratch ({kind})"), n


def _ok_or_refused(rc, what):
    """a call may refuse a capacity with an error code; it may not write past it"""
    L = _L()
    if rc != 0:
        msg = L.lib().cilrs_last_error()
        assert msg, f"{what}: error code without a message"


def _conv_fwd(N, H, W, Cin, Cout, k, s, p, cfg, splitk):
    L = _L()
    lib = L.lib()
    Ho, Wo = out_hw(H, W, k, s, p)
    x, w = R(N, H, W, Cin), R(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    for kind in CAPACITIES:
        g = Guards()
        y = g.buf((N, Ho, Wo, Cout), guard=128 * Cout, name=f"y ({kind})")
        scr, cap = _capacity(g, kind, y.numel())
        g.const(x=x, w=w)
        rc = lib.cilrs_conv2d_fwd(L.ptr(x), L.ptr(w), L.ptr(y), N, H, W, Cin, Cout, k, k, s, p, cfg,
                                  splitk, L.ptr(scr), cap, stream())
        _ok_or_refused(rc, "conv2d_fwd")
        if rc != 0:
            g.finite = []
        g.verify()


def _conv_dgrad(N, H, W, Cin, Cout, k, s, p, cfg, splitk):
    L = _L()
    lib = L.lib()
    Ho, Wo = out_hw(H, W, k, s, p)
    dy, w = R(N, Ho, Wo, Cout), R(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    add = R(N, H, W, Cin)
    for kind in CAPACITIES:
        for addend in (None, add):
            g = Guards()
            dx = g.buf((N, H, W, Cin), guard=128 * Cin, name=f"dx ({kind}, addend {addend is not None})")
            scr, cap = _capacity(g, kind, dx.numel())
            g.const(dy=dy, w=w, addend=addend)
            rc = lib.cilrs_conv2d_dgrad(L.ptr(dy), L.ptr(w), L.ptr(dx), L.ptr(addend), N, H, W, Cin,
                                        Cout, k, k, s, p, cfg, splitk, L.ptr(scr), cap, stream())
            _ok_or_refused(rc, "conv2d_dgrad")
            if rc != 0:
                g.finite = []
            g.verify()


@pytest.mark.parametrize("case,cfg,splitk", FWD_CASES)
def test_conv_fwd_guards(case, cfg, splitk):
    _conv_fwd(*case, cfg, splitk)


@pytest.mark.parametrize("case,cfg,splitk", DGRAD_CASES)
def test_conv_dgrad_guards(case, cfg, splitk):
    _conv_dgrad(*case, cfg, splitk)


@pytest.mark.parametrize("shape", TRUNK_SHAPES)
def test_conv_fwd_dgrad_guards_at_benchmark_batch(shape):
    _conv_fwd(128, *shape, -1, 0)
    _conv_dgrad(128, *shape, -1, 0)


# ---- the same two with the fused BatchNorm reductions ----------------------------------------------
@pytest.mark.parametrize("cfg,splitk", STATS_PLANS)
@pytest.mark.parametrize("case", BOTTLENECK_GUARD_CASES)
def test_conv_fwd_stats_guards(case, cfg, splitk):
    """the column partials land in a buffer of exactly cilrs_bn_partial_floats(Cout) floats, and
    [2][Cout][*nblk] of it is written"""
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    x, w = R(N, H, W, Cin), R(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    npart = lib.cilrs_bn_partial_floats(Cout)
    for kind in CAPACITIES:
        g = Guards()
        y = g.buf((N, Ho, Wo, Cout), guard=128 * Cout, name=f"fwd_stats y ({kind})")
        part = g.buf(npart, guard=npart, name=f"fwd_stats partial ({kind})", finite=False)
        scr, cap = _capacity(g, kind, y.numel())
        nblk = C.c_int(-1)
        g.const(x=x, w=w)
        rc = lib.cilrs_conv2d_fwd_stats(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(part), C.byref(nblk), N, H,
                                        W, Cin, Cout, k, s, p, cfg, splitk, L.ptr(scr), cap, stream())
        _ok_or_refused(rc, "conv2d_fwd_stats")
        if rc != 0:
            g.finite = []
        g.verify()
        if rc == 0:
            assert 0 <= nblk.value and 2 * Cout * nblk.value <= npart
            all_finite(part[:2 * Cout * nblk.value], "fwd_stats partial [2][Cout][nblk]")


@pytest.mark.parametrize("cfg,splitk", STATS_PLANS)
@pytest.mark.parametrize("case", [c for c in BOTTLENECK_GUARD_CASES if c[6] == 1])
def test_conv_dgrad_bnbwd_guards(case, cfg, splitk):
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    M = N * H * W
    dy, w = R(N, Ho, Wo, Cout), R(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    add, bz, by = R(M, Cin), R(M, Cin), R(M, Cin)
    bstats = torch.cat([R(Cin, scale=0.1), torch.rand(Cin, device="cuda") + 0.5, R(2 * Cin)])
    npart = lib.cilrs_bn_partial_floats(Cin)
    for kind in CAPACITIES:
        g = Guards()
        dx = g.buf((M, Cin), guard=128 * Cin, name=f"dgrad_bnbwd dx ({kind})")
        part = g.buf(npart, guard=npart, name=f"dgrad_bnbwd partial ({kind})", finite=False)
        scr, cap = _capacity(g, kind, dx.numel())
        nblk = C.c_int(-1)
        g.const(dy=dy, w=w, addend=add, bwd_z=bz, bwd_y=by, bwd_stats=bstats)
        rc = lib.cilrs_conv2d_dgrad_bnbwd(L.ptr(dy), L.ptr(w), L.ptr(dx), L.ptr(add), L.ptr(bz),
                                          L.ptr(by), L.ptr(bstats), 1, L.ptr(part), C.byref(nblk), N, H,
                                          W, Cin, Cout, k, s, p, cfg, splitk, L.ptr(scr), cap, stream())
        _ok_or_refused(rc, "conv2d_dgrad_bnbwd")
        if rc != 0:
            g.finite = []
        g.verify()
        if rc == 0:
            assert 0 <= nblk.value and 2 * Cin * nblk.value <= npart
            all_finite(part[:2 * Cin * nblk.value], "dgrad_bnbwd partial [2][Cin][nblk]")


# ---- fp32 weight gradient, the stem's three kernels ------------------------------------------------
WGRAD_CASES = (CONV_CASES + [(4, 22, 50, 64, 64, 3, 1, 1)] + [(128,) + s for s in TRUNK_SHAPES]
               + BOTTLENECK_GUARD_CASES)


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_conv_wgrad_guards(case):
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    x, dy = R(N, H, W, Cin), R(N, Ho, Wo, Cout)
    g = Guards()
    dw = g.buf((Cout, k, k, Cin), guard=128 * k * k * Cin, name="dw")
    scr = g.scratch(lib.cilrs_conv2d_wgrad_scratch_floats(N, H, W, Cin, Cout, k, k, s, p), name="slabs")
    g.const(x=x, dy=dy)
    L.check(lib.cilrs_conv2d_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(scr), N, H, W, Cin, Cout, k,
                                   k, s, p, Cin, stream()))
    g.verify()


def test_conv_wgrad_guards_channel_padded_stem():
    """Cin 4 -> 3 kept channels: dw is [64][7][7][3], narrower than the slabs' rows"""
    L = _L()
    lib = L.lib()
    N, H, W = 2, 88, 200
    x4, dy = R(N, H, W, 4), R(N, 44, 100, 64)
    g = Guards()
    dw = g.buf((64, 7, 7, 3), guard=128 * 49 * 4, name="dw")
    scr = g.scratch(lib.cilrs_conv2d_wgrad_scratch_floats(N, H, W, 4, 64, 7, 7, 2, 3), name="slabs")
    g.const(x4=x4, dy=dy)
    L.check(lib.cilrs_conv2d_wgrad(L.ptr(x4), L.ptr(dy), L.ptr(dw), L.ptr(scr), N, H, W, 4, 64, 7, 7,
                                   2, 3, 3, stream()))
    g.verify()


STEM_FWD_SHAPES = [(5, 88, 200), (2, 40, 120), (3, 176, 400), (2, 30, 70), (1, 88, 200), (3, 9, 253),
                   (2, 61, 445), (9, 86, 199), (2, 26, 400), (128, 88, 200)]
STEM_WGRAD_SHAPES = [(3, 88, 200), (2, 176, 400), (1, 88, 200), (9, 86, 199), (2, 26, 400),
                     (128, 88, 200)]
STEM_DGRAD_SHAPES = [(2, 88, 200), (1, 176, 400), (2, 90, 202), (3, 96, 160), (1, 64, 64), (1, 37, 51),
                     (9, 86, 199), (2, 26, 400), (128, 88, 200)]


@pytest.mark.parametrize("shape", STEM_FWD_SHAPES)
def test_stem_conv_fwd_guards(shape):
    L = _L()
    lib = L.lib()
    N, H, W = shape
    Ho, Wo = out_hw(H, W, 7, 2, 3)
    x4, w = R(N, H, W, 4), R(64, 7, 7, 3, scale=147 ** -0.5)
    rows = C.c_int(0)
    g = Guards()
    y = g.buf((N, Ho, Wo, 64), guard=256 * 64, name="y (no partials)")       # 256-pixel tiles
    g.const(x4=x4, w=w)
    L.check(lib.cilrs_stem_conv_fwd(L.ptr(x4), L.ptr(w), L.ptr(y), None, N, H, W, C.byref(rows), stream()))
    g.verify()
    assert rows.value > 0
    g = Guards()
    y2 = g.buf((N, Ho, Wo, 64), guard=256 * 64, name="y")
    part = g.buf((2, 64, rows.value), guard=2 * 64 * rows.value, name="bn_partial [2][64][rows]")
    g.const(x4=x4, w=w)
    L.check(lib.cilrs_stem_conv_fwd(L.ptr(x4), L.ptr(w), L.ptr(y2), L.ptr(part), N, H, W, None, stream()))
    g.verify()
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape", STEM_WGRAD_SHAPES)
def test_stem_conv_wgrad_guards(shape):
    L = _L()
    lib = L.lib()
    N, H, W = shape
    Ho, Wo = out_hw(H, W, 7, 2, 3)
    need = lib.cilrs_stem_conv_wgrad_scratch_floats(N, H, W)
    assert need > 0
    x4, dy = R(N, H, W, 4), R(N, Ho, Wo, 64)
    g = Guards()
    dw = g.buf((64, 7, 7, 3), guard=64 * 160, name="dw")
    scr = g.scratch(need, name="slabs")
    g.const(x4=x4, dy=dy)
    L.check(lib.cilrs_stem_conv_wgrad(L.ptr(x4), L.ptr(dy), L.ptr(dw), L.ptr(scr), need, N, H, W,
                                      stream()))
    g.verify()


@pytest.mark.parametrize("shape", STEM_DGRAD_SHAPES)
@pytest.mark.parametrize("layout", ["nchw_pitched", "nhwc_pitched"])
def test_stem_conv_dgrad_guards_with_gaps_between_rows(shape, layout):
    """dx with non-contiguous strides: every image row is followed by pad elements that hold the
    guard pattern (NCHW: rows of W floats with pitch W + 3; NHWC: rows of 3 W floats, pitch 3 W + 5)"""
    L = _L()
    lib = L.lib()
    N, H, W = shape
    Ho, Wo = out_hw(H, W, 7, 2, 3)
    dy, w = R(N, Ho, Wo, 64), R(64, 7, 7, 3, scale=0.1)
    g = Guards()
    if layout == "nchw_pitched":
        ld = W + 3
        full, logical = g.rows(N * 3 * H, W, ld, guard=16 * ld, name="dx rows")
        sn, sc, sh, sw = 3 * H * ld, H * ld, ld, 1
    else:
        ld = 3 * W + 5
        full, logical = g.rows(N * H, 3 * W, ld, guard=16 * ld, name="dx rows")
        sn, sc, sh, sw = H * ld, 1, ld, 3
    g.const(dy=dy, w=w)
    L.check(lib.cilrs_stem_conv_dgrad(L.ptr(dy), L.ptr(w), L.ptr(full), sn, sc, sh, sw, N, H, W,
                                      stream()))
    g.verify()


# ---- Winograd F(2x2, 3x3) --------------------------------------------------------------------------
@pytest.mark.parametrize("case", WINO_CASES)
def test_wino_guards(case):
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout = case
    M = N * H * W
    x, w = R(N, H, W, Cin), R(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5)
    nU = lib.cilrs_conv2d_wino_scratch_floats(Cin, Cout)
    # forward: filter transform + convolution
    g = Guards()
    y = g.buf((N, H, W, Cout), guard=256 * Cout, name="wino_fwd y")          # 64 tiles of 2x2 pixels
    U = g.scratch(nU, name="wino_fwd U")
    g.const(x=x, w=w)
    L.check(lib.cilrs_conv2d_wino_fwd(L.ptr(x), L.ptr(w), L.ptr(y), N, H, W, Cin, Cout, L.ptr(U), stream()))
    g.verify()
    # the filter transform alone (forward form), then the convolution on the ready U, with an addend
    g = Guards()
    U0 = g.buf(nU, guard=nU, name="filter_transform U")
    g.const(w=w)
    L.check(lib.cilrs_wino_filter_transform(L.ptr(w), L.ptr(U0), Cin, Cout, 0, stream()))
    g.verify()
    add = R(N, H, W, Cout)
    g = Guards()
    y = g.buf((N, H, W, Cout), guard=256 * Cout, name="wino_pre y")
    g.const(x=x, U=U0, add=add)
    L.check(lib.cilrs_conv2d_wino_pre(L.ptr(x), L.ptr(U0), L.ptr(y), L.ptr(add), N, H, W, Cin, Cout,
                                      stream()))
    g.verify()
    # the train step's launch plan: slabs for up to four parts per tile, BatchNorm column partials
    g = Guards()
    y = g.buf((N, H, W, Cout), guard=256 * Cout, name="wino_split y")
    slabs = g.scratch(4 * M * Cout, name="wino_split slabs")
    npart = lib.cilrs_bn_partial_floats(Cout)
    part = g.buf(npart, guard=npart, name="wino_split bn_partial", finite=False)
    cs, rows = C.c_int(0), C.c_int(0)
    g.const(x=x, U=U0, add=add)
    L.check(lib.cilrs_conv2d_wino_split(L.ptr(x), L.ptr(U0), L.ptr(y), L.ptr(add), L.ptr(part), N, H, W,
                                        Cin, Cout, L.ptr(slabs), slabs.numel(), C.byref(cs),
                                        C.byref(rows), stream()))
    g.verify()
    assert 0 < rows.value and 2 * Cout * rows.value <= npart
    all_finite(part[:2 * Cout * rows.value], "wino_split bn_partial [2][Cout][rows]")
    # folded eval-mode BatchNorm epilogue
    scale, shift = R(Cout), R(Cout)
    g = Guards()
    y = g.buf((N, H, W, Cout), guard=256 * Cout, name="wino_fold_fwd y")
    U = g.scratch(nU, name="wino_fold_fwd U")
    g.const(x=x, w=w, scale=scale, shift=shift, add=add)
    L.check(lib.cilrs_conv2d_wino_fold_fwd(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(scale), L.ptr(shift),
                                           L.ptr(add), 1, 1, N, H, W, Cin, Cout, L.ptr(U), stream()))
    g.verify()
    if Cin % 64:
        return
    # data gradient (the roles of the channel counts swap) and its filter transform
    dy, addx = R(N, H, W, Cout), R(N, H, W, Cin)
    g = Guards()
    Ud = g.buf(nU, guard=nU, name="filter_transform U (dgrad)")
    g.const(w=w)
    L.check(lib.cilrs_wino_filter_transform(L.ptr(w), L.ptr(Ud), Cin, Cout, 1, stream()))
    g.verify()
    g = Guards()
    dx = g.buf((N, H, W, Cin), guard=256 * Cin, name="wino_dgrad dx")
    U = g.scratch(nU, name="wino_dgrad U")
    g.const(dy=dy, w=w, addx=addx)
    L.check(lib.cilrs_conv2d_wino_dgrad(L.ptr(dy), L.ptr(w), L.ptr(dx), L.ptr(addx), N, H, W, Cin, Cout,
                                        L.ptr(U), stream()))
    g.verify()
    # weight gradient in the transform domain
    nsc = lib.cilrs_conv2d_wino_wgrad_scratch_floats(N, H, W, Cin, Cout)
    g = Guards()
    dw = g.buf((Cout, 3, 3, Cin), guard=64 * 9 * Cin, name="wino_wgrad dw")
    sc2 = g.scratch(nsc, name="wino_wgrad slabs")
    g.const(x=x, dy=dy)
    L.check(lib.cilrs_conv2d_wino_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), N, H, W, Cin, Cout, L.ptr(sc2),
                                        nsc, stream()))
    g.verify()


# ---- 16-bit convolutions ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV16_CASES)
@pytest.mark.parametrize("bf16", [1, 0])
def test_conv16_guards(case, bf16):
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    M = N * Ho * Wo
    x, w, dy = R(N, H, W, Cin), R(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5), R(N, Ho, Wo, Cout)
    add = R(N, H, W, Cin)
    n16 = lib.cilrs_conv2d_16_scratch_halfs(N, H, W, Cin, Cout, k, s, p)
    nmt = (M + 63) // 64
    g = Guards()
    y = g.buf((N, Ho, Wo, Cout), guard=128 * Cout, name="fwd_16 y")
    part = g.buf((2, Cout, nmt), guard=2 * Cout * nmt, name="fwd_16 bn_partial [2][Cout][ceil(M/64)]")
    s16 = g.scratch(n16, I16, name="fwd_16 scratch16")
    g.const(x=x, w=w)
    L.check(lib.cilrs_conv2d_fwd_16(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(part), N, H, W, Cin, Cout, k,
                                    s, p, bf16, L.ptr(s16), stream()))
    g.verify()
    for addend in (None, add):
        g = Guards()
        dx = g.buf((N, H, W, Cin), guard=128 * Cin, name="dgrad_16 dx")
        s16 = g.scratch(n16, I16, name="dgrad_16 scratch16")
        g.const(dy=dy, w=w, addend=addend)
        L.check(lib.cilrs_conv2d_dgrad_16(L.ptr(dy), L.ptr(w), L.ptr(dx), L.ptr(addend), N, H, W, Cin,
                                          Cout, k, s, p, bf16, L.ptr(s16), stream()))
        g.verify()
    g = Guards()
    dw = g.buf((Cout, k, k, Cin), guard=128 * k * k * Cin, name="wgrad_16 dw")
    s16 = g.scratch(n16, I16, name="wgrad_16 scratch16")
    s32 = g.scratch(lib.cilrs_conv2d_wgrad_16_scratch_floats(N, H, W, Cin, Cout, k, s, p),
                    name="wgrad_16 scratch32")
    g.const(x=x, dy=dy)
    L.check(lib.cilrs_conv2d_wgrad_16(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(s32), N, H, W, Cin, Cout,
                                      k, s, p, bf16, L.ptr(s16), stream()))
    g.verify()


@pytest.mark.parametrize("case", CONV16T_CASES)
def test_conv16_train_guards(case):
    L = _L()
    lib = L.lib()
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    M = N * Ho * Wo
    nmt = (M + 63) // 64
    x, w = R(N, H, W, Cin, dtype=BF16), R(Cout, k, k, Cin, dtype=BF16, scale=(k * k * Cin) ** -0.5)
    add, bz, by = R(M, Cout, dtype=BF16), R(M, Cout, dtype=BF16), R(M, Cout, dtype=BF16)
    bstats = torch.cat([R(Cout, scale=0.1), torch.rand(Cout, device="cuda") + 0.5])
    rows = C.c_int(0)

    def run(g, y16, y32, addend, part, z, yy, st, relu, bpart):
        g.const(x=x, w=w, addend=addend, bwd_z=z, bwd_y=yy, bwd_stats=st)
        L.check(lib.cilrs_conv2d_train_16(L.ptr(x), L.ptr(w), L.ptr(y16), L.ptr(y32), L.ptr(addend),
                                          L.ptr(part), L.ptr(z), L.ptr(yy), L.ptr(st), relu,
                                          L.ptr(bpart), N, H, W, Cin, Ho, Wo, Cout, k, s, p, 0, 1,
                                          C.byref(rows), stream()))
        g.verify()

    # forward form: rounded result + BatchNorm statistics
    g = Guards()
    y = g.buf((M, Cout), BF16, guard=128 * Cout, name="train_16 y16")
    part = g.buf((2, Cout, nmt), guard=2 * Cout * nmt, name="train_16 bn_partial", finite=False)
    run(g, y, None, None, part, None, None, None, 0, None)
    assert rows.value in (nmt, (M + 127) // 128)
    all_finite(part.flatten()[:2 * Cout * rows.value], "train_16 bn_partial [2][Cout][rows]")
    # data-gradient form: addend + BatchNorm-backward reductions
    g = Guards()
    y = g.buf((M, Cout), BF16, guard=128 * Cout, name="train_16 y16 (+ addend)")
    bpart = g.buf((2, Cout, nmt), guard=2 * Cout * nmt, name="train_16 bwd_partial", finite=False)
    run(g, y, None, add, None, bz, by, bstats, 1, bpart)
    all_finite(bpart.flatten()[:2 * Cout * rows.value], "train_16 bwd_partial [2][Cout][rows]")
    # fp32 result
    g = Guards()
    y32 = g.buf((M, Cout), guard=128 * Cout, name="train_16 y32")
    run(g, None, y32, add, None, None, None, None, 0, None)


INFER16_CASES = RAGGED_CASES + BOTTLENECK_CASES + [CONV_CASES[-1]]


@pytest.mark.parametrize("case", INFER16_CASES)
@pytest.mark.parametrize("bf16", [1, 0])
def test_conv16_infer_guards(case, bf16):
    L = _L()
    lib = L.lib()
    T = BF16 if bf16 else F16
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = out_hw(H, W, k, s, p)
    x = R(N, H, W, Cin, dtype=T).relu_()
    w = R(Cout, k, k, Cin, dtype=T, scale=(k * k * Cin) ** -0.5)
    bias, res = R(Cout, scale=0.2), R(N, Ho, Wo, Cout, dtype=T)
    for tile in ((0, 128) if Cout % 128 == 0 else (0,)):
        for residual in (None, res):
            g = Guards()
            y = g.buf((N, Ho, Wo, Cout), T, guard=128 * Cout, name=f"infer_16 y16 (tile {tile or 64})")
            g.const(x=x, w=w, bias=bias, residual=residual)
            L.check(lib.cilrs_conv2d_infer_16(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(residual), L.ptr(y),
                                              N, H, W, Cin, Cout, k, s, p, 1, bf16, tile, stream()))
            g.verify()


@pytest.mark.parametrize("N,H,W", [(5, 88, 200), (2, 176, 400), (1, 88, 200), (3, 9, 253),
                                   (2, 61, 445), (2, 30, 70)])
@pytest.mark.parametrize("bf16", [1, 0])
def test_stem_infer16_guards(N, H, W, bf16):
    L = _L()
    lib = L.lib()
    T = BF16 if bf16 else F16
    Ho, Wo = out_hw(H, W, 7, 2, 3)
    w, stats = R(64, 7, 7, 3, scale=147 ** -0.5), R(256)
    g = Guards()
    w16 = g.buf((64, 7, 8, 4), T, guard=64 * 7 * 8 * 4, name="stem_fold w16")
    bias = g.buf(64, guard=64, name="stem_fold bias")
    g.const(w=w, stats=stats)
    L.check(lib.cilrs_stem_fold_16(L.ptr(w), L.ptr(stats), L.ptr(w16), L.ptr(bias), bf16, stream()))
    g.verify()
    x4 = R(N, H, W, 4)
    g = Guards()
    z = g.buf((N, Ho, Wo, 64), T, guard=128 * 64, name="stem_infer_16 z16")
    g.const(x4=x4, w16=w16, bias=bias)
    L.check(lib.cilrs_stem_infer_16(L.ptr(x4), L.ptr(w16), L.ptr(bias), L.ptr(z), N, H, W, bf16, stream()))
    g.verify()


@pytest.mark.parametrize("N,H,W", [(1, 7, 9), (3, 8, 8), (2, 44, 100)])
@pytest.mark.parametrize("bf16", [1, 0])
def test_maxpool_infer16_guards(N, H, W, bf16):
    L = _L()
    lib = L.lib()
    T = BF16 if bf16 else F16
    Ho, Wo = out_hw(H, W, 3, 2, 1)
    x = R(N, H, W, 64, dtype=T)
    g = Guards()
    out = g.buf((N, Ho, Wo, 64), T, guard=Wo * 64, name="maxpool_infer_16 out")
    g.const(x=x)
    L.check(lib.cilrs_maxpool_infer_16(L.ptr(x), L.ptr(out), N, H, W, 64, bf16, stream()))
    g.verify()


@pytest.mark.parametrize("HW", [21, 66])
@pytest.mark.parametrize("Cc", [512, 2048])
@pytest.mark.parametrize("bf16", [1, 0])
def test_avgpool_infer16_guards(HW, Cc, bf16):
    L = _L()
    lib = L.lib()
    T = BF16 if bf16 else F16
    N, ld = 3, Cc + 128
    x = R(N, HW, Cc, dtype=T)
    g = Guards()
    full, _ = g.rows(N, Cc, ld, guard=ld, name="avgpool_infer_16 out")
    g.const(x=x)
    L.check(lib.cilrs_avgpool_infer_16(L.ptr(x), L.ptr(full), N, HW, Cc, ld, bf16, stream()))
    g.verify()


# ---- BatchNorm and pooling ---------------------------------------------------------------------------
BN_CASES = [(3 * 22 * 50, 64), (5 * 275, 128), (2 * 78, 256), (21, 512), (8 * 4400, 64),
            (1, 64), (63, 64), (65, 64)]
BN16_CASES = [(2 * 22 * 50, 64), (8 * 11 * 25, 128), (3 * 6 * 13, 256), (77, 2048), (16 * 44 * 100, 256),
              (1, 64), (63, 64), (65, 64)]


def _bn_params(Cc):
    gamma, beta = torch.rand(Cc, device="cuda") + 0.5, torch.rand(Cc, device="cuda") - 0.5
    rm, rv = torch.rand(Cc, device="cuda") - 0.5, torch.rand(Cc, device="cuda") + 0.5
    return gamma, beta, rm, rv


@pytest.mark.parametrize("M,Cc", BN_CASES)
@pytest.mark.parametrize("relu,res", [(1, True), (0, False)])
def test_bn_train_fwd_bwd_guards(M, Cc, relu, res):
    L = _L()
    lib = L.lib()
    y, dz = R(M, Cc, scale=1.7) + 0.3, R(M, Cc)
    resid = R(M, Cc) if res else None
    gamma, beta, rm0, rv0 = _bn_params(Cc)
    npart = lib.cilrs_bn_partial_floats(Cc)
    g = Guards()
    z = g.buf((M, Cc), guard=64 * Cc, name="bn_train_fwd z")
    stats = g.buf(4 * Cc, guard=4 * Cc, name="bn_train_fwd stats [4C]")
    part = g.scratch(npart, name="bn_train_fwd partial")
    rm = g.buf(Cc, fill=None, guard=Cc, name="running_mean")
    rv = g.buf(Cc, fill=None, guard=Cc, name="running_var")
    nbt = g.buf(1, I64, fill=0, guard=1, name="num_batches_tracked")
    rm.copy_(rm0), rv.copy_(rv0)
    g.const(y=y, gamma=gamma, beta=beta, residual=resid)
    L.check(lib.cilrs_bn_train_fwd(L.ptr(y), M, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv),
                                   L.ptr(nbt), 0.1, 1e-5, L.ptr(resid), relu, L.ptr(stats), L.ptr(part),
                                   L.ptr(z), stream()))
    g.verify()
    all_finite(rm, "running_mean"), all_finite(rv, "running_var")
    assert int(nbt) == 1
    g = Guards()
    dy = g.buf((M, Cc), guard=64 * Cc, name="bn_bwd dy")
    gout = g.buf((M, Cc), guard=64 * Cc, name="bn_bwd g_out")
    dgamma = g.buf(Cc, guard=Cc, name="bn_bwd dgamma")
    dbeta = g.buf(Cc, guard=Cc, name="bn_bwd dbeta")
    coef = g.buf(3 * Cc, guard=3 * Cc, name="bn_bwd coef [3C]")
    part = g.scratch(npart, name="bn_bwd partial")
    g.const(dz=dz, z=z, y=y, gamma=gamma, stats=stats)
    L.check(lib.cilrs_bn_bwd(L.ptr(dz), L.ptr(z), L.ptr(y), M, Cc, L.ptr(gamma), L.ptr(stats), relu,
                             L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), L.ptr(part), L.ptr(dy),
                             L.ptr(gout), stream()))
    g.verify()


@pytest.mark.parametrize("M", [1100, 1, 63, 65])
def test_bn_eval_fwd_guards(M):
    L = _L()
    lib = L.lib()
    Cc = 64
    y = R(M, Cc)
    gamma, beta, rm, rv = _bn_params(Cc)
    g = Guards()
    z = g.buf((M, Cc), guard=64 * Cc, name="bn_eval_fwd z")
    stats = g.buf(4 * Cc, guard=4 * Cc, name="bn_eval_fwd stats [4C]")
    g.const(y=y, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)
    L.check(lib.cilrs_bn_eval_fwd(L.ptr(y), M, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), 1e-5,
                                  None, 1, L.ptr(stats), L.ptr(z), stream()))
    g.verify()


@pytest.mark.parametrize("M,Cc", [(35, 64), (1100, 128), (312, 512), (42, 2048), (1, 64), (63, 64),
                                  (65, 64)])
@pytest.mark.parametrize("relu", [0, 1])
def test_bn_bwd_frozen_guards(M, Cc, relu):
    L = _L()
    lib = L.lib()
    dz, z, gamma, stats = R(M, Cc), R(M, Cc).relu_(), R(Cc), R(4 * Cc)
    g = Guards()
    dy = g.buf((M, Cc), guard=64 * Cc, name="bn_bwd_frozen dy")
    gout = g.buf((M, Cc), guard=64 * Cc, name="bn_bwd_frozen g_out")
    g.const(dz=dz, z=z, gamma=gamma, stats=stats)
    L.check(lib.cilrs_bn_bwd_frozen(L.ptr(dz), L.ptr(z) if relu else None, M, Cc, L.ptr(gamma),
                                    L.ptr(stats), relu, L.ptr(dy), L.ptr(gout), stream()))
    g.verify()


@pytest.mark.parametrize("N,H,W", [(2, 44, 100), (1, 7, 9), (3, 8, 8), (1, 19, 26)])
def test_maxpool_and_pool_frozen_guards(N, H, W):
    L = _L()
    lib = L.lib()
    Cc = 64
    Ho, Wo = out_hw(H, W, 3, 2, 1)
    x, dout = R(N, H, W, Cc).relu_(), R(N, Ho, Wo, Cc)
    g = Guards()
    out = g.buf((N, Ho, Wo, Cc), guard=Wo * Cc, name="maxpool_fwd out")
    am = g.buf((N, Ho, Wo, Cc), U8, fill=255, guard=Wo * Cc, name="maxpool_fwd argmax (uint8)")
    g.const(x=x)
    L.check(lib.cilrs_maxpool_fwd(L.ptr(x), L.ptr(out), L.ptr(am), N, H, W, Cc, stream()))
    g.verify()
    assert int(am.max()) <= 8                                   # every argmax written: a tap 0..8
    g = Guards()
    dx = g.buf((N, H, W, Cc), guard=W * Cc, name="maxpool_bwd dx")
    g.const(dout=dout, argmax=am)
    L.check(lib.cilrs_maxpool_bwd(L.ptr(dout), L.ptr(am), L.ptr(dx), N, H, W, Cc, stream()))
    g.verify()
    # the stem's frozen form: scatter + mask + scale, every element of dy written
    y, gamma, stats = R(N, H, W, Cc), R(Cc), R(4 * Cc)
    g = Guards()
    dy = g.buf((N, H, W, Cc), guard=2 * W * Cc, name="bn_bwd_pool_frozen dy")
    g.const(dpool=dout, argmax=am, y=y, gamma=gamma, stats=stats)
    L.check(lib.cilrs_bn_bwd_pool_frozen(L.ptr(dout), L.ptr(am), L.ptr(y), N, H, W, Cc, L.ptr(gamma),
                                         L.ptr(stats), L.ptr(dy), stream()))
    g.verify()


@pytest.mark.parametrize("M,Cc", BN16_CASES)
def test_bn16_train_fwd_bwd_guards(M, Cc):
    L = _L()
    lib = L.lib()
    y, res, dz = R(M, Cc, dtype=BF16, scale=1.5), R(M, Cc, dtype=BF16), R(M, Cc, dtype=BF16)
    gamma, beta, rm0, rv0 = _bn_params(Cc)
    npart = lib.cilrs_bn_partial_floats(Cc)
    g = Guards()
    z = g.buf((M, Cc), BF16, guard=64 * Cc, name="bn16_train_fwd z16")
    stats = g.buf(4 * Cc, guard=4 * Cc, name="bn16_train_fwd stats [4C]")
    part = g.scratch(npart, name="bn16_train_fwd partial")
    rm = g.buf(Cc, fill=None, guard=Cc, name="running_mean")
    rv = g.buf(Cc, fill=None, guard=Cc, name="running_var")
    nbt = g.buf(1, I64, fill=0, guard=1, name="num_batches_tracked")
    rm.copy_(rm0), rv.copy_(rv0)
    g.const(y=y, gamma=gamma, beta=beta, residual=res)
    L.check(lib.cilrs_bn16_train_fwd(L.ptr(y), M, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv),
                                     L.ptr(nbt), 0.1, 1e-5, L.ptr(res), 1, L.ptr(stats), L.ptr(part),
                                     L.ptr(z), 0, stream()))
    g.verify()
    all_finite(rm, "running_mean"), all_finite(rv, "running_var")
    g = Guards()
    dy = g.buf((M, Cc), BF16, guard=64 * Cc, name="bn16_bwd dy16")
    gout = g.buf((M, Cc), BF16, guard=64 * Cc, name="bn16_bwd g_out16")
    dgamma = g.buf(Cc, guard=Cc, name="bn16_bwd dgamma")
    dbeta = g.buf(Cc, guard=Cc, name="bn16_bwd dbeta")
    coef = g.buf(3 * Cc, guard=3 * Cc, name="bn16_bwd coef [3C]")
    part = g.scratch(npart, name="bn16_bwd partial")
    g.const(dz=dz, z=z, y=y, gamma=gamma, stats=stats)
    L.check(lib.cilrs_bn16_bwd(L.ptr(dz), L.ptr(z), L.ptr(y), M, Cc, L.ptr(gamma), L.ptr(stats), 1,
                               L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), L.ptr(part), L.ptr(dy),
                               L.ptr(gout), 0, stream()))
    g.verify()


# ---- heads, loss, optimiser ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,fin,fout", LINEAR_CASES)
def test_linear_fwd_bwd_guards(B, fin, fout):
    """x and dx live inside wider rows (pitch in + 4): the four pad columns of every dx row hold the
    guard pattern, like the bands before and after it"""
    L = _L()
    lib = L.lib()
    ld = fin + 4
    xw, w, b = R(B, ld), R(fout, fin, scale=max(1.0, fin ** 0.5) ** -1), R(fout)
    g = Guards()
    y = g.buf((B, fout), guard=128 * fout, name="linear_fwd y")
    g.const(x=xw, w=w, bias=b)
    L.check(lib.cilrs_linear_fwd(L.ptr(xw), L.ptr(w), L.ptr(b), L.ptr(y), B, fin, fout, ld, fout, 1,
                                 stream()))
    g.verify()
    dy, act = R(B, fout), R(B, fin)
    g = Guards()
    dxf, _ = g.rows(B, fin, ld, guard=128 * ld, name="linear_bwd dx (pitch in + 4)")
    dw = g.buf((fout, fin), guard=128 * fin, name="linear_bwd dw")
    db = g.buf(fout, guard=fout, name="linear_bwd db")
    g.const(dy=dy, x=xw, w=w, act=act)
    L.check(lib.cilrs_linear_bwd(L.ptr(dy), L.ptr(xw), L.ptr(w), L.ptr(act), 2.0, L.ptr(dxf), L.ptr(dw),
                                 L.ptr(db), B, fin, fout, fout, ld, ld, fin, stream()))
    g.verify()


@pytest.mark.parametrize("rows,cols,ld", [(128, 512, 516), (5, 3, 7), (33, 257, 260)])
def test_dropout_guards(rows, cols, ld):
    L = _L()
    g = Guards()
    full, logical = g.rows(rows, cols, ld, fill=1.0, guard=ld, name="dropout matrix (ld > cols)")
    L.check(L.lib().cilrs_dropout(L.ptr(full), rows, cols, ld, 0.5, 1234, 3, stream()))
    g.verify()
    assert bool(((logical == 0) | (logical == 2.0)).all())


@pytest.mark.parametrize("B", [3, 257])
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_guards(B, kind):
    L = _L()
    pc, tc, ps, ts = R(B, 3), R(B, 3), R(B), R(B)
    w4 = (C.c_float * 4)(0.5, 0.45, 0.05, 0.1)
    g = Guards()
    out = g.buf(6, guard=6, name="loss_out [6]")
    dpc = g.buf((B, 3), guard=3 * B, name="dcontrols")
    dps = g.buf(B, guard=B, name="dpred_speed")
    g.const(controls=pc, target_controls=tc, pred_speed=ps, target_speed=ts)
    L.check(L.lib().cilrs_loss_fwd_bwd(L.ptr(pc), L.ptr(tc), L.ptr(ps), L.ptr(ts), B, kind, w4, 0.125,
                                       L.ptr(dpc), L.ptr(dps), L.ptr(out), stream()))
    g.verify()


@pytest.mark.parametrize("n", [4, 1024, 4 * (1024 * 256 + 1)])
def test_grad_sqnorm_guards(n):
    L = _L()
    lib = L.lib()
    gr = R(n)
    g = Guards()
    scr = g.scratch(lib.cilrs_sqnorm_scratch_bytes(), U8, name="sqnorm scratch (bytes)")
    out2 = g.buf(2, guard=2, name="sqnorm out2")
    g.const(grads=gr)
    L.check(lib.cilrs_grad_sqnorm(L.ptr(gr), n, 1.0, L.ptr(scr), L.ptr(out2), stream()))
    g.verify()


ARENA_SIZES = [4, 4 * 257, 4 * (4096 * 256 + 3)]      # the last: a second grid-stride trip, ragged end


def _arena(g, n, name, positive=False):
    v = g.buf(n, fill=None, guard=4 * 1024, name=name)
    v.copy_(torch.rand(n, device="cuda") if positive else torch.randn(n, device="cuda"))
    return v


@pytest.mark.parametrize("n", ARENA_SIZES)
@pytest.mark.parametrize("groups", [0, 1, 3])
def test_adam_step_guards(n, groups):
    """groups = 0: cilrs_adam_step; 1 / 3: cilrs_adam_step_groups with that many ranges"""
    L = _L()
    lib = L.lib()
    if groups > n // 4:
        groups = n // 4
    gr, clip = R(n), torch.tensor([2.0, 0.5], device="cuda")
    g = Guards()
    p, m, v = _arena(g, n, "params"), _arena(g, n, "exp_avg"), _arena(g, n, "exp_avg_sq", True)
    p0 = p.clone()
    g.const(grads=gr, clip_out2=clip)
    if groups == 0:
        L.check(lib.cilrs_adam_step(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, 2e-4, 0.9, 0.999, 1e-8,
                                    1e-4, 3, L.ptr(clip), 0.5, stream()))
    else:
        n4 = n // 4
        ends = [4 * ((i + 1) * n4 // groups) for i in range(groups)]
        assert ends[-1] == n and all(e > 0 for e in ends)
        e_ = (C.c_size_t * groups)(*ends)
        lrs = (C.c_double * groups)(*[2e-4 * (i + 1) for i in range(groups)])
        steps = (C.c_int64 * groups)(*[3 + i for i in range(groups)])
        L.check(lib.cilrs_adam_step_groups(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, groups, e_, lrs,
                                           steps, 0.9, 0.999, 1e-8, 1e-4, L.ptr(clip), 0.5, stream()))
    g.verify()
    all_finite(p, "params"), all_finite(m, "exp_avg"), all_finite(v, "exp_avg_sq")
    # every element takes its step (an update smaller than half a spacing of p leaves a few as they
    # were: m close to zero), the ragged end of the second grid-stride trip included
    assert float((p != p0).float().mean()) > 0.99
    assert float((p[-1024:] != p0[-1024:]).float().mean()) > 0.9 and bool((m[-4:] != 0).all())


@pytest.mark.parametrize("n", ARENA_SIZES)
def test_scale_guards(n):
    L = _L()
    clip = torch.tensor([2.0, 0.5], device="cuda")
    g = Guards()
    x = _arena(g, n, "x")
    x0 = x.clone()
    g.const(clip_out2=clip)
    L.check(L.lib().cilrs_scale(L.ptr(x), n, L.ptr(clip), 0.5, stream()))
    g.verify()
    assert torch.equal(x, x0 * 0.25)


@pytest.mark.parametrize("B", [1, 65, 300])
def test_eval_accumulate_guards(B):
    L = _L()
    lib = L.lib()
    nacc = lib.cilrs_eval_acc_doubles()
    pc, tc, ps, ts = R(B, 3), R(B, 3), R(B), R(B)
    cmd = torch.randint(0, 4, (B,), device="cuda")
    g = Guards()
    acc = g.buf(nacc, F64, fill=0.0, guard=nacc, name="eval accumulator (doubles)")
    err = g.buf(B, guard=B, name="steer_abs_err")
    g.const(controls=pc, pred_speed=ps, target_controls=tc, target_speed=ts, command=cmd)
    L.check(lib.cilrs_eval_accumulate(L.ptr(pc), L.ptr(ps), L.ptr(tc), L.ptr(ts), L.ptr(cmd), B,
                                      L.ptr(acc), L.ptr(err), stream()))
    g.verify()
    all_finite(acc, "eval accumulator")
    assert float(acc[0]) == B


@pytest.mark.parametrize("channels_last", [False, True])
def test_saliency_map_guards(channels_last):
    L = _L()
    B, H, W = 1, 37, 51
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    d = R(B, 3, H, W).contiguous(memory_format=fmt)
    g = Guards()
    heat = g.buf((B, H, W), guard=H * W, name="heat")
    heat8 = g.buf((B, H, W), U8, fill=77, guard=H * W, name="heat_u8")
    peak = g.buf(B, guard=B, name="peak")
    g.const(dimage=d)
    L.check(L.lib().cilrs_saliency_map(L.ptr(d), *d.stride(), B, H, W, None, L.ptr(heat), L.ptr(heat8),
                                       L.ptr(peak), stream()))
    g.verify()


def _aug_params(batch):
    from cilrs_mi355 import data as D
    p = D.draw_aug_params(np.random.default_rng(16), 16)[:batch]
    return p, torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(batch, -1)).cuda()


def test_augment_u8_guards():
    L = _L()
    B, H, W = 6, 88, 200
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=U8, device="cuda")
    _, pdev = _aug_params(B)
    g = Guards()
    outf = g.buf((B, H, W, 3), guard=H * W * 3, name="augment out_f32")
    out8 = g.buf((B, H, W, 3), U8, fill=7, guard=H * W * 3, name="augment out_u8")
    g.const(frames=frames, params=pdev)
    L.check(L.lib().cilrs_augment_u8(L.ptr(frames), L.ptr(pdev), B, H, W, L.ptr(outf), L.ptr(out8),
                                     stream()))
    g.verify()


def test_batch_assemble_guards():
    L = _L()
    n, B, H, W = 37, 16, 88, 200
    cache = torch.randint(0, 256, (n, H, W, 3), dtype=U8, device="cuda")
    speed, targets = torch.rand(n, device="cuda"), torch.rand(n, 3, device="cuda")
    command = torch.randint(0, 4, (n,), device="cuda")
    index = torch.tensor([36, 5, 0, 17, 5, 36, 9, 22, 0, 1, 30, 29, 5, 12, 35, 3], device="cuda")
    _, pdev = _aug_params(B)
    g = Guards()
    outf = g.buf((B, H, W, 3), guard=H * W * 3, name="assemble out_f32")
    out8 = g.buf((B, H, W, 3), U8, fill=7, guard=H * W * 3, name="assemble out_u8")
    ospd = g.buf(B, guard=B, name="assemble out_speed")
    ocmd = g.buf(B, I64, fill=-1, guard=B, name="assemble out_command")
    otgt = g.buf((B, 3), guard=3 * B, name="assemble out_targets")
    g.const(cache=cache, speed=speed, command=command, targets=targets, index=index, params=pdev)
    L.check(L.lib().cilrs_batch_assemble(L.ptr(cache), n, L.ptr(speed), L.ptr(command), L.ptr(targets),
                                         L.ptr(index), L.ptr(pdev), B, H, W, L.ptr(outf), L.ptr(out8),
                                         L.ptr(ospd), L.ptr(ocmd), L.ptr(otgt), stream()))
    g.verify()
    assert int(ocmd.min()) >= 0
