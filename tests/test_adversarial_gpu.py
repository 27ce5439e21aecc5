"""FGSM / PGD on the device: the four kernels of csrc/adversarial.hip, Predictor.adversarial,
evaluate.adversarial_sweep and the adversarial train step of Trainer.

Gates:
  start, step, direction, quantize   torch.equal to the fp32 numpy statement of tests/_adversarial.py
                                     (single-rounded fp32 operations and integer work only), in
                                     contiguous NCHW, in the channels-last view and with the gradient
                                     in strides of its own; outputs NaN-filled inside the guard bands
                                     of tests/_guards.py, inputs checked unwritten; two runs bit-identical
  Predictor.adversarial              eps = 0 is the clean frame and saliency's `out`; linf <= ceil(eps);
                                     |dev| never shrinks with more steps; equal to the same launches driven
                                     by hand; out_adv within 1e-4 of the CPU oracle on the returned bytes;
                                     one FGSM step against the float64 oracle's own FGSM within
                                     max(4x |fp32 CPU oracle - float64 oracle|, 5e-3 |dev64|), the gate of
                                     tests/test_saliency_gpu.py for the same gradient
  adversarial_sweep                  eps = 0 is `evaluate` on those frames; the control row; JSON
  Trainer                            adv_eps = 0 is the plain step; one adversarial step is torch.equal to
                                     the composition from the public pieces; adv_every; EMA; world-1
                                     data-parallel routes; refusals
"""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import _adversarial as A
import _ema as E
import cilrs_oracle as O
from _guards import Inputs, guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5), (2, 7, 33), (2, 8, 12), (1, 88, 200)]     # scalar tails, 16-byte paths, the frame
EPS = [0.0, 0.5, 2.0, 300.0]
LAYOUTS = ("nchw", "nhwc")
NAN = float("nan")


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def place(cpu, layout, name, dtype=torch.float32):
    """A logical NCHW [B,3,H,W] device tensor in `layout` inside guard bands, NaN-filled (cpu None)
    or holding `cpu`; returns (tensor, guard check)."""
    B, _, H, W = cpu.shape if not isinstance(cpu, tuple) else cpu
    flat, check = guarded(B * 3 * H * W, dtype, NAN, name=name)
    t = flat.view(B, 3, H, W) if layout == "nchw" else flat.view(B, H, W, 3).permute(0, 3, 1, 2)
    if not isinstance(cpu, tuple):
        t.copy_(torch.from_numpy(np.ascontiguousarray(cpu)))
    return t, check


def strides_of(B, H, W, layout):
    return (3 * H * W, H * W, W, 1) if layout == "nchw" else (3 * H * W, 1, 3 * W, 3)


def _data(B, H, W, seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[0, 0, 0] = (0, 255, 0)
    frames[-1, -1, -1] = (255, 0, 255)
    x = A.preprocess(frames)
    g = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    flat = g.reshape(-1)
    flat[::11] = 0.0
    flat[1::13] = -0.0
    flat[2::17] = NAN
    flat[3::19] = float("inf")
    flat[4::23] = float("-inf")
    return frames, x, g


def floats(values):
    return None if values is None else (C.c_float * len(values))(*values)


def same(t, want):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


def bits(t):
    return t.contiguous().view(-1).view(torch.int32).cpu()


def call_start(x, eps255, seed, rng, out):
    L = _L()
    B, _, H, W = x.shape
    L.check(L.lib().cilrs_adv_start(L.ptr(x), *x.stride(), B, H, W, eps255, floats(A.CHAN_SCALE), seed,
                                    floats(rng), L.ptr(out), *out.stride(), stream()))


def call_step(x, xa, g, alpha255, eps255, row_dir, improved, best, rng):
    L = _L()
    B, _, H, W = x.shape
    z = (0, 0, 0, 0)
    L.check(L.lib().cilrs_adv_step(
        L.ptr(x), L.ptr(xa), *x.stride(), L.ptr(g), *(g.stride() if g is not None else z), B, H, W,
        alpha255, eps255, floats(A.CHAN_SCALE), L.ptr(row_dir), L.ptr(improved), L.ptr(best),
        *(best.stride() if best is not None else z), floats(rng), stream()))


# ---- 1. cilrs_adv_start ----------------------------------------------------------------------------
@pytest.mark.parametrize("eps255", EPS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_start_is_the_fp32_statement(B, H, W, eps255):
    _, x_np, _ = _data(B, H, W, 1 + H)
    seed = 0x1234567890ABCDEF
    for lx, lo in (("nchw", "nchw"), ("nhwc", "nhwc"), ("nchw", "nhwc"), ("nhwc", "nchw")):
        for rng in (None, A.RANGE6):
            x, check_x = place(x_np, lx, "x")
            out, check_out = place((B, 3, H, W), lo, "x_adv")
            ins = Inputs(x=x)
            call_start(x, eps255, seed, rng, out)
            check_out()
            check_x()
            ins.check()
            want = A.start_ref(x_np, eps255, seed, rng)
            assert same(out, want), (lx, lo, rng is not None)
            if eps255 == 0:
                assert torch.equal(bits(out), bits(x))               # a copy, bit for bit
            else:
                assert not same(out, x_np)
            again, _ = place((B, 3, H, W), lo, "x_adv again")
            call_start(x, eps255, seed, rng, again)
            assert torch.equal(bits(again), bits(out))               # run to run, layout to layout


# ---- 2. cilrs_adv_step -----------------------------------------------------------------------------
@pytest.mark.parametrize("eps255", EPS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_step_is_the_fp32_statement(B, H, W, eps255):
    _, x_np, g_np = _data(B, H, W, 2 + W)
    xa_np = A.start_ref(x_np, eps255, 77)
    alpha255 = 0.25 * eps255 + 0.125
    rd_np = np.array([-1.0, 1.0][:B], dtype=np.float32)
    imp_np = np.array([1, 0][:B], dtype=np.int32)
    cases = [("nchw", "nchw", "nchw", None, False), ("nhwc", "nhwc", "nhwc", rd_np, True),
             ("nchw", "nhwc", "nchw", rd_np, True), ("nhwc", "nchw", "nchw", None, True),
             ("nchw", "nchw", "nhwc", rd_np, True)]
    for lx, lg, lb, rd, copy in cases:
        for rng in (None, A.RANGE6):
            x, check_x = place(x_np, lx, "x")
            xa, check_xa = place(xa_np, lx, "x_adv")
            g, check_g = place(g_np, lg, "g")
            best, check_best = place((B, 3, H, W), lb, "best")
            row_dir = torch.from_numpy(rd).cuda() if rd is not None else None
            improved = torch.from_numpy(imp_np).cuda() if copy else None
            ins = Inputs(x=x, g=g, row_dir=row_dir, improved=improved)
            call_step(x, xa, g, alpha255, eps255, row_dir, improved, best if copy else None, rng)
            for chk in (check_x, check_xa, check_g, check_best):
                chk()
            ins.check()
            want, want_best = A.step_ref(x_np, xa_np, g_np, alpha255, eps255, rd,
                                         imp_np if copy else None,
                                         np.full_like(x_np, NAN) if copy else None, rng)
            tag = (lx, lg, lb, rd is not None, copy, rng is not None)
            assert same(xa, want), tag
            got_best = best.cpu().numpy()
            if copy:
                # the conditional copy reads the PRE-step iterate; other frames are left unwritten
                assert np.array_equal(got_best[imp_np != 0], xa_np[imp_np != 0]), tag
                assert np.isnan(got_best[imp_np == 0]).all(), tag
                assert np.array_equal(np.isnan(want_best), np.isnan(got_best))
            else:
                assert np.isnan(got_best).all(), tag
            e = A.per_channel(eps255)
            assert (want >= x_np - e).all() and (want <= x_np + e).all()
            xb, _ = place(xa_np, lx, "x_adv again")
            call_step(x, xb, g, alpha255, eps255, row_dir, improved, best if copy else None, rng)
            assert torch.equal(bits(xb), bits(xa))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_step_with_alpha_zero_leaves_every_bit_and_still_copies(B, H, W):
    _, x_np, g_np = _data(B, H, W, 5)
    xa_np = A.start_ref(x_np, 2.0, 3)
    xa_np.reshape(-1)[::7] = -0.0                            # bits a float round trip could lose
    imp_np = np.array([0, 1][-B:], dtype=np.int32)
    for layout in LAYOUTS:
        x, _ = place(x_np, layout, "x")
        xa, check_xa = place(xa_np, layout, "x_adv")
        best, check_best = place((B, 3, H, W), layout, "best")
        improved = torch.from_numpy(imp_np).cuda()
        before = bits(xa)
        call_step(x, xa, None, 0.0, 2.0, None, improved, best, A.RANGE6)     # g NULL is allowed here
        check_xa()
        check_best()
        assert torch.equal(bits(xa), before)
        got = best.cpu().numpy()
        assert np.array_equal(got[imp_np != 0].view(np.int32), xa_np[imp_np != 0].view(np.int32))
        assert np.isnan(got[imp_np == 0]).all()
        call_step(x, xa, None, 0.0, 2.0, None, None, None, None)             # nothing to do at all
        assert torch.equal(bits(xa), before)


# ---- 3. cilrs_adv_direction ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 300])
def test_direction_is_the_fp32_statement(B):
    L = _L()
    rng = np.random.default_rng(B)
    c, rc = (rng.standard_normal((B, 3)).astype(np.float32) for _ in range(2))
    s, rs = (rng.standard_normal(B).astype(np.float32) for _ in range(2))
    c[0, 0] = rc[0, 0]                                       # a tie at zero for w = steer
    if B >= 5:
        c[1, 0], c[2, 0], s[3] = NAN, float("inf"), float("-inf")
    prev = (0.5 * rng.standard_normal(B)).astype(np.float32)
    for w4 in ((1.0, 0.0, 0.0, 0.0), (0.5, -1.0, 0.25, 2.0)):
        for first in (1, 0):
            dev_t = [torch.from_numpy(a).cuda() for a in (c, s, rc, rs)]
            dev, chk_dev = guarded(B, name="dev")
            row_dir, chk_rd = guarded(B, name="row_dir")
            best, chk_best = guarded(B, name="best_dev")
            improved, chk_imp = guarded(B, torch.int32, -7, name="improved")
            if not first:
                best.copy_(torch.from_numpy(prev))
            ins = Inputs(c=dev_t[0], s=dev_t[1], rc=dev_t[2], rs=dev_t[3])
            L.check(L.lib().cilrs_adv_direction(*[L.ptr(t) for t in dev_t], floats(w4), B, first,
                                                L.ptr(dev), L.ptr(best), L.ptr(row_dir),
                                                L.ptr(improved), stream()))
            for chk in (chk_dev, chk_rd, chk_best, chk_imp):
                chk()
            ins.check()
            w_dev, w_best, w_rd, w_imp = A.direction_ref(c, s, rc, rs, w4, first, prev)
            got = dev.cpu().numpy()
            assert np.array_equal(got, w_dev, equal_nan=True)
            assert same(best, w_best) and same(row_dir, w_rd) and same(improved, w_imp)
            assert np.isfinite(best.cpu().numpy()).all()


# ---- 4. cilrs_adv_quantize -------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_quantize_is_the_fp32_statement(B, H, W):
    L = _L()
    frames_np, x_np, g_np = _data(B, H, W, 9)
    xa_np, _ = A.step_ref(x_np, A.start_ref(x_np, 8.0, 4), g_np, 3.0, 8.0)
    xa_np.reshape(-1)[5::29] = NAN
    xa_np.reshape(-1)[6::31] = 1e9
    xa_np.reshape(-1)[7::37] = -1e9
    want, want_linf = A.quantize_ref(xa_np, frames_np)
    for layout in LAYOUTS:
        for with_linf in (True, False):
            xa, _ = place(xa_np, layout, "x_adv")
            frames = torch.from_numpy(frames_np).cuda()
            out, chk_out = guarded(B * H * W * 3, torch.uint8, 99, name="out_u8")
            linf, chk_linf = guarded(B, torch.int32, -1, name="linf")
            ins = Inputs(x_adv=xa, frames=frames)
            L.check(L.lib().cilrs_adv_quantize(L.ptr(xa), *xa.stride(), L.ptr(frames), B, H, W,
                                               L.ptr(out), L.ptr(linf) if with_linf else None,
                                               stream()))
            chk_out()
            chk_linf()
            ins.check()
            assert same(out.view(B, H, W, 3), want), layout
            if with_linf:
                assert same(linf, want_linf), layout
            else:
                assert bool((linf == -1).all())
    # integer eps inside the range: no byte moves more than eps, 0 and 255 included
    for eps in (1, 8):
        xa_np, _ = A.step_ref(x_np, x_np, g_np, float(eps), float(eps), None, None, None, A.RANGE6)
        xa, _ = place(xa_np, "nhwc", "x_adv")
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        linf = torch.empty(B, dtype=torch.int32, device="cuda")
        L.check(L.lib().cilrs_adv_quantize(L.ptr(xa), *xa.stride(), L.ptr(torch.from_numpy(frames_np).cuda()),
                                           B, H, W, L.ptr(out), L.ptr(linf), stream()))
        diff = (out.cpu().int() - torch.from_numpy(frames_np).int()).abs()
        assert int(diff.max()) == eps and torch.equal(linf.cpu(), diff.view(B, -1).amax(1).int())


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch():
    L = _L()
    lib = L.lib()
    B, H, W = 2, 8, 12
    _, x_np, g_np = _data(B, H, W, 1)
    x, _ = place(x_np, "nchw", "x")
    g, _ = place(g_np, "nchw", "g")
    xa, chk_xa = place((B, 3, H, W), "nchw", "x_adv")
    best, chk_best = place((B, 3, H, W), "nchw", "best")
    out, chk_out = guarded(B * H * W * 3, torch.uint8, 99, name="out_u8")
    st = x.stride()
    cs = floats(A.CHAN_SCALE)
    z = (0, 0, 0, 0)
    imp = torch.ones(B, dtype=torch.int32, device="cuda")

    def refused(rc, what):
        assert rc != 0
        msg = lib.cilrs_last_error()
        assert msg and what.encode() in msg, (what, msg)

    p = L.ptr
    refused(lib.cilrs_adv_start(p(x), *st, B, H, W, -1.0, cs, 0, None, p(xa), *st, stream()), "eps255")
    refused(lib.cilrs_adv_start(p(x), *st, B, H, W, NAN, cs, 0, None, p(xa), *st, stream()), "eps255")
    refused(lib.cilrs_adv_start(p(x), *st, B, H, W, 1.0, cs, 0, None, None, *st, stream()), "NULL")
    refused(lib.cilrs_adv_start(p(x), *st, B, H, W, 1.0, cs, 0, None, p(xa), st[0], st[1], -1, 1,
                                stream()), "negative stride")
    refused(lib.cilrs_adv_start(p(x), *st, 1 << 15, 1 << 8, 1 << 8, 1.0, cs, 0, None, p(xa), *st,
                                stream()), "2^30")
    refused(lib.cilrs_adv_step(p(x), p(xa), *st, None, *z, B, H, W, 1.0, 1.0, cs, None, p(imp),
                               p(best), *st, None, stream()), "only when alpha255 = 0")
    refused(lib.cilrs_adv_step(p(x), p(xa), *st, p(g), *st, B, H, W, float("inf"), 1.0, cs, None,
                               p(imp), p(best), *st, None, stream()), "alpha255")
    refused(lib.cilrs_adv_step(p(x), p(xa), *st, p(g), *st, B, H, W, 1.0, -2.0, cs, None, p(imp),
                               p(best), *st, None, stream()), "eps255")
    refused(lib.cilrs_adv_step(p(x), p(xa), *st, p(g), -1, 1, 1, 1, B, H, W, 1.0, 1.0, cs, None,
                               p(imp), p(best), *st, None, stream()), "negative stride")
    refused(lib.cilrs_adv_quantize(p(x), *st, None, B, H, W, p(out), p(imp), stream()),
            "needs the clean frames")
    refused(lib.cilrs_adv_quantize(p(x), st[0], st[1], st[2], -1, None, B, H, W, p(out), None,
                                   stream()), "negative stride")
    for chk, buf in ((chk_xa, xa), (chk_best, best)):
        chk()
        assert bool(torch.isnan(buf).all())                  # nothing was written
    chk_out()
    assert bool((out == 99).all()) and bool((imp == 1).all())
    # the engine's own checks, before the library is reached
    from cilrs_mi355 import CILRS
    eng = CILRS(4, 0.0).cuda().engine()
    with pytest.raises(RuntimeError, match="same strides"):
        eng.run_adv_step(x, place(x_np, "nhwc", "x_adv")[0], g, 1.0, 1.0, A.CHAN_SCALE)
    with pytest.raises(RuntimeError, match="float32"):
        eng.run_adv_start(x.double(), 1.0, A.CHAN_SCALE, 0, xa)
    with pytest.raises(RuntimeError, match="improved"):
        eng.run_adv_step(x, xa, g, 1.0, 1.0, A.CHAN_SCALE, improved=imp.float(), best=best)
    with pytest.raises(RuntimeError, match="out_u8"):
        eng.run_adv_quantize(x, out_u8=torch.empty(B, H, W, 4, dtype=torch.uint8, device="cuda"))


# ====================================================================================================
# Predictor.adversarial: B = 2, 88 x 200, the oracle's portable weights
# ====================================================================================================
H88, W200 = 88, 200
SPEEDS, CMDS = [12.0, 55.0], [2, 0]
STEER = (1.0, 0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def frames2():
    return O.synthetic_batch(2, seed=81)[4]


def make_model(seed=0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def predictor():
    from cilrs_mi355.predict import Predictor
    return Predictor(make_model(), batch=2)


@pytest.fixture(scope="module")
def oracles():
    return {torch.float64: O.build_oracle(0).double().eval(), torch.float32: O.build_oracle(0).eval()}


def oracle_out(orc, x, dtype):
    spd = torch.tensor([min(s / O.SPEED_NORM, 1.0) for s in SPEEDS], dtype=dtype)
    pc, ps = orc(x.to(dtype), spd, torch.tensor(CMDS))
    return pc, ps.reshape(-1)


def test_eps_zero_is_the_clean_frame_and_saliencys_out(predictor):
    u8 = frames2()
    want = predictor.saliency(u8, SPEEDS, CMDS)[0]
    for goal in ("deviate", "increase"):
        clean, adv, frames, info = predictor.adversarial(u8, SPEEDS, CMDS, eps=0.0, steps=2, goal=goal)
        assert np.array_equal(clean, want)
        assert np.array_equal(frames, u8) and frames.dtype == np.uint8
        assert (info["dev"] == 0).all() and (info["linf"] == 0).all()
        assert info["eps"] == 0.0 and info["steps"] == 2 and info["alpha"] == 0.0
        assert np.abs(adv - clean)[:, :3].max() <= 1e-6      # the same frames through the same forward


@pytest.mark.parametrize("eps", [1, 2.5, 8])
def test_no_byte_moves_more_than_eps_levels(predictor, eps):
    u8 = frames2()
    _, _, frames, info = predictor.adversarial(u8, SPEEDS, CMDS, eps=eps, steps=2, seed=3)
    diff = np.abs(frames.astype(np.int32) - u8.astype(np.int32)).reshape(2, -1).max(1)
    assert np.array_equal(info["linf"], diff) and (diff <= math.ceil(eps)).all() and (diff >= 1).all()


def test_more_steps_never_lose_deviation_and_the_result_is_reproducible(predictor):
    u8 = frames2()
    kw = dict(eps=2.0, alpha=0.75, goal="deviate", seed=5)
    one = predictor.adversarial(u8, SPEEDS, CMDS, steps=1, **kw)
    three = predictor.adversarial(u8, SPEEDS, CMDS, steps=3, **kw)
    again = predictor.adversarial(u8, SPEEDS, CMDS, steps=3, **kw)
    print("|dev| steps=1", np.abs(one[3]["dev"]), "steps=3", np.abs(three[3]["dev"]))
    assert (np.abs(three[3]["dev"]) >= np.abs(one[3]["dev"])).all()  # shared prefix, the best is kept
    assert (np.abs(three[3]["dev"]) > 0).all()
    for a, b in zip(three[:3], again[:3]):
        assert np.array_equal(a, b)
    for k in ("dev", "dev_u8", "linf"):
        assert np.array_equal(three[3][k], again[3][k])
    other = predictor.adversarial(u8, SPEEDS, CMDS, steps=3, **dict(kw, seed=6))
    assert not np.array_equal(other[2], three[2]) and np.array_equal(other[0], three[0])


def test_the_public_call_is_the_same_launches_driven_by_hand(predictor):
    from cilrs_mi355.adversarial import CHAN_SCALE, RANGE6
    u8 = frames2()
    eps, alpha, steps, seed = 2.0, 0.75, 2, 9
    clean, adv, frames, info = predictor.adversarial(u8, SPEEDS, CMDS, eps=eps, alpha=alpha,
                                                     steps=steps, goal="deviate", seed=seed)
    eng, dev = predictor.eng, predictor.eng.device
    f = torch.from_numpy(u8).to(dev)
    spd = torch.tensor([s / 90.0 for s in SPEEDS], dtype=torch.float64).float().to(dev)
    cmd = torch.tensor(CMDS, device=dev)
    dc = torch.tensor([STEER[:3]] * 2, device=dev)
    ds = torch.zeros(2, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    x, xa, best, g = (torch.full((2, 3, H88, W200), NAN, **f32) for _ in range(4))
    d, bd, rd = (torch.empty(2, **f32) for _ in range(3))
    imp = torch.empty(2, dtype=torch.int32, device=dev)
    c0, s0, _ = eng.run_forward_frozen_u8(f, spd, cmd)
    eng.run_attr_samples(f, None, 0, 1, 0, 1, 0.0, 0, out=x)
    eng.run_adv_start(x, eps, CHAN_SCALE, seed, xa, RANGE6)
    best.copy_(xa)
    for k in range(steps + 1):
        c, s, pl = eng.run_forward_frozen(xa, spd, cmd)
        eng.run_adv_direction(c, s, c0, s0, STEER, k == 0, d, bd, rd, imp)
        if k == steps:
            eng.run_adv_step(x, xa, None, 0.0, eps, CHAN_SCALE, None, imp, best)
            break
        eng.run_backward(pl, dc, ds, data_only=True, segments=(0, 6))
        eng.run_input_grads(pl, g, None)
        eng.run_adv_step(x, xa, g, alpha, eps, CHAN_SCALE, rd, imp, best, RANGE6)
    linf = torch.empty(2, dtype=torch.int32, device=dev)
    q = eng.run_adv_quantize(best, f, None, linf)
    cq, sq, _ = eng.run_forward_frozen_u8(q, spd, cmd)
    torch.cuda.synchronize()
    assert np.array_equal(frames, q.cpu().numpy())
    assert np.array_equal(info["dev"], bd.cpu().numpy())
    assert np.array_equal(info["linf"], linf.cpu().numpy())
    assert np.array_equal(adv[:, :3], cq.cpu().numpy()) and np.array_equal(clean[:, :3], c0.cpu().numpy())
    assert np.array_equal(info["dev_u8"], (cq[:, 0] - c0[:, 0]).cpu().numpy())
    assert torch.equal(x.cpu(), torch.from_numpy(A.preprocess(u8)))  # the clean input is the preprocessing


def test_out_adv_is_the_oracle_on_the_returned_bytes_and_fgsm_beats_random_signs(predictor, oracles):
    """FGSM at eps = 2 moves the steer farther than a random-sign step of the same size, on every
    frame.  The CPU fp32 oracle alone, frames synthetic_batch(2, seed=81), control seed 0:
    FGSM steer deviation (+0.178, +0.212), random-sign control (-0.0037, -0.0009)."""
    from cilrs_mi355.adversarial import CHAN_SCALE, RANGE6
    u8 = frames2()
    clean, adv, frames, info = predictor.adversarial(u8, SPEEDS, CMDS, eps=2.0, steps=1,
                                                     goal="increase")
    assert info["alpha"] == 2.0 and (info["linf"] == 2).all()
    orc = oracles[torch.float32]
    with torch.no_grad():
        pc, ps = oracle_out(orc, torch.from_numpy(A.preprocess(frames)), torch.float32)
        pc0, _ = oracle_out(orc, torch.from_numpy(A.preprocess(u8)), torch.float32)
    assert np.abs(adv[:, :3] - pc.numpy()).max() <= 1e-4
    assert np.abs(adv[:, 3] - ps.numpy() * 90.0).max() <= 90e-4
    # the control, by hand: one step of size eps along the sign of cilrs_adv_start's draw
    eng, dev = predictor.eng, predictor.eng.device
    f = torch.from_numpy(u8).to(dev)
    x = eng.run_attr_samples(f, None, 0, 1, 0, 1, 0.0, 0)
    sign = eng.run_adv_start(torch.zeros_like(x), 1.0, CHAN_SCALE, 0, torch.empty_like(x))
    xa = x.clone()
    eng.run_adv_step(x, xa, sign, 2.0, 2.0, CHAN_SCALE, None, None, None, RANGE6)
    linf = torch.empty(2, dtype=torch.int32, device=dev)
    q = eng.run_adv_quantize(xa, f, None, linf)
    spd = torch.tensor([s / 90.0 for s in SPEEDS], dtype=torch.float64).float().to(dev)
    cq, _, _ = eng.run_forward_frozen_u8(q, spd, torch.tensor(CMDS, device=dev))
    control = cq[:, 0].cpu().numpy() - clean[:, 0]
    want_sign = A.start_ref(np.zeros((2, 3, H88, W200), np.float32), 1.0, 0)
    assert same(sign, want_sign) and (linf.cpu() == 2).all()
    with torch.no_grad():
        pcc, _ = oracle_out(orc, torch.from_numpy(A.preprocess(q.cpu().numpy())), torch.float32)
    o_fgsm = (pc[:, 0] - pc0[:, 0]).numpy()
    o_ctrl = (pcc[:, 0] - pc0[:, 0]).numpy()
    print("steer deviation: FGSM", info["dev_u8"], "control", control, "| oracle", o_fgsm, o_ctrl)
    assert (np.abs(o_fgsm) > np.abs(o_ctrl)).all()           # the oracle alone says so
    assert (np.abs(info["dev_u8"]) > np.abs(control)).all()
    assert (info["dev_u8"] > 0).all()                        # goal="increase"


def test_one_fgsm_step_against_the_float64_oracles_own_fgsm(predictor, oracles):
    u8 = frames2()
    eps = 0.25
    _, _, _, info = predictor.adversarial(u8, SPEEDS, CMDS, eps=eps, steps=1, goal="increase",
                                          random_start=False)
    ref = {}
    for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        x = torch.from_numpy(A.preprocess(u8, npdt)).requires_grad_()
        pc, _ = oracle_out(oracles[dt], x, dt)
        pc[:, 0].sum().backward()
        xa, _ = A.step_ref(x.detach().numpy(), x.detach().numpy(), x.grad.numpy(), eps, eps, None,
                           None, None, A.RANGE6, npdt)
        with torch.no_grad():
            pa, _ = oracle_out(oracles[dt], torch.from_numpy(xa), dt)
        ref[dt] = (pa[:, 0] - pc[:, 0]).detach().double().numpy()
    d64, d32 = ref[torch.float64], ref[torch.float32]
    gate = np.maximum(4.0 * np.abs(d32 - d64), 5e-3 * np.abs(d64))
    err = np.abs(info["dev"].astype(np.float64) - d64)
    print(f"FGSM eps={eps}: dev {info['dev']} float64 oracle {d64} fp32 CPU oracle {d32} gate {gate}")
    assert (d64 > 0).all() and (err <= gate).all(), (err, gate)


def test_the_persistent_tick_is_not_disturbed_and_misuse_raises_before_any_launch():
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(1, seed=71)[4]
    m = make_model()
    pr = Predictor(m)                                        # B = 1: the persistent predictor
    assert pr.persistent
    before = pr.predict_batch(u8, [20.0], [3])
    a = pr.adversarial(u8, [20.0], [3], output="throttle", eps=2.0, steps=2, seed=1)
    b = pr.adversarial(u8, [20.0], [3], output="throttle", eps=2.0, steps=2, seed=1)
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3]))
    e = pr.adversarial(u8, [20.0], [3], eps=1.0, steps=1, goal="error", targets=[[0.1, 0.5, 0.0]])
    assert e[3]["dev"].shape == (1,) and e[3]["linf"][0] == 1
    after = pr.predict_batch(u8, [20.0], [3])
    assert np.array_equal(before, after)
    assert pr.persistent and pr.degraded_ticks_left == 0 and pr.barrier_timeouts == 0
    eng = m.engine()
    params, epoch = eng.params.clone(), eng.weights_epoch
    for bad in (dict(goal="untargeted"), dict(output="steering"), dict(eps=-1.0), dict(steps=0),
                dict(alpha=float("nan")), dict(seed=-1), dict(goal="error"),
                dict(targets=[[0.0, 0.0, 0.0]]),
                dict(goal="error", targets=[[0.0, 0.0, 0.0]], output="speed")):
        with pytest.raises(ValueError):
            pr.adversarial(u8, [10.0], [1], **bad)
    with pytest.raises(RuntimeError, match="out of range"):
        pr.adversarial(u8, [10.0], [4])
    with pytest.raises(RuntimeError, match="network resolution"):
        pr.adversarial(np.zeros((1, 600, 800, 4), dtype=np.uint8), [10.0], [1])
    eng.train_precision = "bf16"
    try:
        with pytest.raises(RuntimeError, match="fp32 plans only"):
            pr.adversarial(u8, [10.0], [1])
    finally:
        eng.train_precision = "fp32"
    torch.cuda.synchronize()
    assert torch.equal(eng.params, params) and eng.weights_epoch == epoch


# ====================================================================================================
# evaluate.adversarial_sweep: a synthetic DeviceDataset of 8 frames
# ====================================================================================================
def test_sweep_eps_zero_is_evaluate_and_the_control_row_is_there(tmp_path):
    from cilrs_mi355 import CachedBatchLoader, DeviceDataset
    from cilrs_mi355.evaluate import evaluate, write_adversarial_sweep
    _, spd, cmd, tgt, u8 = O.synthetic_batch(8, seed=90)
    ds = DeviceDataset.from_tensors(torch.from_numpy(u8).cuda(), spd.cuda(), cmd.cuda(), tgt.cuda())
    m = make_model()
    idx = np.arange(8)
    path = tmp_path / "sweep.json"
    rep = write_adversarial_sweep(path, m, ds, idx, eps=(0, 2), steps=2, batch=8, seed=1)
    plain = evaluate(m, CachedBatchLoader(ds, idx, 8, train=False))
    assert rep["clean"] == plain
    zero = rep["eps"][0.0]
    for row in ("attack", "control"):
        assert zero[row]["report"] == plain, row
        assert zero[row]["linf_max"] == 0 and zero[row]["steer_mae"] == plain["overall_metrics"]["Steer"]["MAE"]
    two = rep["eps"][2.0]
    assert set(two) == {"attack", "control"} and two["attack"]["linf_max"] == 2 == two["control"]["linf_max"]
    print("eps=2 steer MAE: attack", two["attack"]["steer_mae"], "control", two["control"]["steer_mae"],
          "clean", plain["overall_metrics"]["Steer"]["MAE"])
    # goal="error" ascends |steer - label|: the attack's mean error is above the control's
    assert two["attack"]["dev_mean"] > two["control"]["dev_mean"]
    assert two["attack"]["steer_mae"] > two["control"]["steer_mae"]
    for row in two.values():
        assert set(row) == {"report", "steer_mae", "dev_mean", "dev_max", "share_over_0.1", "linf_max",
                            "linf_mean"}
        assert 0.0 <= row["share_over_0.1"] <= 1.0 and row["dev_max"] >= row["dev_mean"] >= 0
    with open(path) as fh:
        assert json.load(fh) == json.loads(json.dumps(rep))
    with pytest.raises(ValueError):
        write_adversarial_sweep(path, m, ds, idx, goal="increase")
    with pytest.raises(ValueError):
        write_adversarial_sweep(path, m, ds, idx, eps=(-1,))


# ====================================================================================================
# Trainer: B = 4 synthetic batches, portable weights
# ====================================================================================================
@pytest.fixture(scope="module")
def weights():
    from cilrs_mi355 import CILRS
    return O.portable_state_dict(CILRS(4, 0.0).state_dict(), 0)


def train_model(weights, dropout=0.0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=dropout)
    m.load_state_dict(weights, strict=True)
    return m.cuda()


@functools.lru_cache(maxsize=None)
def batches(k, seed0=70):
    return [[t.cuda() for t in O.synthetic_batch(4, seed=seed0 + i)[:4]] for i in range(k)]


def cfg_with(base, **kw):
    from cilrs_mi355 import TrainConfig
    return TrainConfig(**{**base.__dict__, **kw})


def snapshot(tr):
    return dict(params=tr.eng.params.cpu(), exp_avg=tr.exp_avg.cpu(), exp_avg_sq=tr.exp_avg_sq.cpu(),
                bn=tr.eng.bn.cpu(), nbt=tr.eng.nbt.cpu(), loss=tr.loss_buf[:6].cpu())


def assert_same_state(a, b, what):
    sa, sb = snapshot(a), snapshot(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs"


def composed_adv_step(tr, batch, cfg, call, sample_weight=None, row_loss=None):
    """One adversarial step from the public pieces on a PLAIN Trainer: start, forward, loss, data
    backward, input grads, step (BatchNorm buffers saved and put back around them), then a plain
    step on x_adv, which draws the same dropout seed.  -> x_adv"""
    from cilrs_mi355.adversarial import CHAN_SCALE, RANGE6
    from cilrs_mi355.train import adv_alpha, adv_seed, dropout_seed
    imgs, spds, cmds, tgts = batch
    eng = tr.eng
    assert tr.cfg.adv_eps == 0.0
    tr.model.train()
    seed = dropout_seed(torch.initial_seed(), tr._seed_calls + 1, 0) if cfg.dropout > 0 else 0
    x_adv, grad = torch.empty_like(imgs), torch.empty_like(imgs)
    assert x_adv.stride() == imgs.stride()
    rng = RANGE6 if cfg.adv_clamp else None
    bn, nbt = eng.bn.clone(), eng.nbt.clone()
    eng.run_adv_start(imgs, cfg.adv_eps if cfg.adv_random_start else 0.0, CHAN_SCALE,
                      adv_seed(torch.initial_seed(), call, 0), x_adv, rng)
    c, s, pl = eng.run_forward_ft(x_adv, spds, cmds, 0, 0, cfg.dropout, seed)
    first = torch.zeros(8, device=imgs.device)
    _, dc, dp = tr.loss(c, tgts, s, spds, out=first, sample_weight=sample_weight, row_loss=row_loss)
    eng.run_backward(pl, dc, dp, data_only=True)
    eng.run_input_grads(pl, grad, None)
    eng.run_adv_step(imgs, x_adv, grad, adv_alpha(cfg), cfg.adv_eps, CHAN_SCALE, None, None, None, rng)
    eng.bn.copy_(bn)
    eng.nbt.copy_(nbt)
    tr.train_step(x_adv, spds, cmds, tgts, sample_weight=sample_weight)
    return x_adv, first


ONE_STEP = {
    "random-start": (dict(), False, False),
    "no-random-start": (dict(adv_random_start=False), False, False),
    "sample-weight": (dict(adv_alpha=1.0), True, False),
    "dropout-clamp-channels-last": (dict(dropout=0.5, adv_clamp=True, grad_clip=1.0), False, True),
}


@pytest.mark.parametrize("case", list(ONE_STEP))
def test_one_adversarial_step_is_the_composition(weights, case):
    from cilrs_mi355 import CONFIG_A, Trainer
    kw, weighted, channels_last = ONE_STEP[case]
    cfg = cfg_with(CONFIG_A, adv_eps=2.0, **kw)
    plain = cfg_with(cfg, adv_eps=0.0)
    batch = list(batches(1)[0])
    if channels_last:
        batch[0] = batch[0].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert batch[0].stride() == (3 * H88 * W200, 1, 3 * W200, 3)
    sw = torch.tensor([0.5, 2.0, 1.0, 0.25], device="cuda") if weighted else None
    rl_a, rl_b = (torch.full((4,), NAN, device="cuda") if weighted else None for _ in range(2))
    ta, tb = Trainer(train_model(weights, cfg.dropout), cfg), Trainer(train_model(weights, cfg.dropout), plain)
    before = snapshot(ta)
    out = ta.train_step(*batch, sample_weight=sw, row_loss=rl_a)
    x_adv, first = composed_adv_step(tb, batch, cfg, 1, sw, rl_b)
    torch.cuda.synchronize()
    assert out is ta.loss_buf and ta.adv_steps == 1 and ta.step_count == tb.step_count == 1
    assert_same_state(ta, tb, case)
    assert torch.equal(ta.sam_loss_buf[:6], first[:6]), "the first pass's loss"
    assert ta._seed_calls == tb._seed_calls == (1 if cfg.dropout > 0 else 0)
    if weighted:
        assert torch.equal(rl_a, rl_b) and bool(torch.isfinite(rl_a).all())     # the first pass's
    # x_adv is inside the eps ball and not the clean batch; one batch was counted
    e = torch.from_numpy(A.per_channel(2.0)).cuda()
    # (x +- e_c are fp32 bounds: the difference may exceed e_c by a rounding of |x| + e_c < 3)
    assert bool(((x_adv - batch[0]).abs() <= e + 3 * 2.0 ** -23).all()) and not torch.equal(x_adv, batch[0])
    assert bool((ta.eng.nbt.cpu() - before["nbt"] == 1).all())
    assert not torch.equal(snapshot(ta)["params"], before["params"])
    # and it is not the plain step on the clean batch
    tc = Trainer(train_model(weights, cfg.dropout), plain)
    tc.train_step(*batch, sample_weight=sw)
    assert not torch.equal(tc.eng.params, ta.eng.params)


def test_adv_off_is_the_plain_step(weights):
    from cilrs_mi355 import CONFIG_A, TrainConfig, Trainer
    spelled = cfg_with(CONFIG_A, adv_eps=0.0, adv_alpha=None, adv_random_start=True, adv_every=1,
                       adv_clamp=False)
    assert spelled == TrainConfig()
    out = []
    for cfg in (CONFIG_A, cfg_with(spelled, adv_every=3, adv_clamp=True)):      # eps = 0: still off
        tr = Trainer(train_model(weights), cfg)
        for b in batches(2):
            tr.train_step(*b)
        assert tr.adv_steps == 0 and not tr._adv_bufs and tr._bn_snapshot is None
        out.append(snapshot(tr))
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


def test_adv_every_two_over_three_steps_and_ema_rides_on_it(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    data = batches(3)
    cfg = cfg_with(CONFIG_A, adv_eps=1.0, adv_every=2, ema_decay=0.9)
    ta = Trainer(train_model(weights), cfg)
    tb = Trainer(train_model(weights), cfg_with(cfg, adv_eps=0.0))
    ema = ta.eng.params.cpu()
    want = [1, 1, 2]
    for t, b in enumerate(data):
        ta.train_step(*b)
        if t % 2 == 0:
            composed_adv_step(tb, b, cfg, want[t])
        else:
            tb.train_step(*b)
        assert ta.adv_steps == want[t]
        assert_same_state(ta, tb, f"step {t + 1}")
        ema = E.step32(ema, ta.eng.params.cpu(), E.weight32(0.9, t + 1, True))
        assert ta.ema_updates == t + 1 and torch.equal(ta.ema.cpu(), ema), f"EMA update {t + 1}"
    assert ta.step_count == 3 and ta.adv_steps == 2


def test_data_parallel_routes_equal_the_single_gpu_route(weights, tmp_path):
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer
    cfg = cfg_with(CONFIG_A, adv_eps=2.0)
    data = batches(2)
    out = {}
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for bucket in (True, False):
            tr = Trainer(train_model(weights), cfg, process_group=dist.group.WORLD)
            tr.bucket_optimizer = bucket
            collectives = []
            for b in data:
                tr.train_step(*b)
                collectives.append(tr.reducer.collectives)
            torch.cuda.synchronize()
            assert tr.step_count == 2 and tr.adv_steps == 2
            assert collectives == [3, 6]                     # the first pass takes no collective
            out[bucket] = snapshot(tr)
    finally:
        dist.destroy_process_group()
    single = Trainer(train_model(weights), cfg)
    for b in data:
        single.train_step(*b)
    out["single"] = snapshot(single)
    for route in (False, "single"):
        for k in out[True]:
            assert torch.equal(out[True][k], out[route][k]), f"{k}: bucket route != {route}"


def test_refused_with_sam_and_behind_a_fine_tuning_cut(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    with pytest.raises(ValueError, match="sam_rho"):
        Trainer(train_model(weights), cfg_with(CONFIG_A, adv_eps=2.0, sam_rho=0.05))
    m = train_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, adv_eps=2.0))
    m.train()
    m.freeze("layer1")
    state, counts = snapshot(tr), (tr.step_count, tr.adv_steps, tr._seed_calls, tr.eng.weights_epoch)
    with pytest.raises(RuntimeError, match="image gradient stops at the cut"):
        tr.train_step(*batches(1)[0])
    torch.cuda.synchronize()
    now = snapshot(tr)
    assert all(torch.equal(now[k], state[k]) for k in now)
    assert counts == (tr.step_count, tr.adv_steps, tr._seed_calls, tr.eng.weights_epoch)
    # what cilrs_net_input_grads itself refuses surfaces with its message
    eng = tr.eng
    imgs, spds, cmds, _ = batches(1)[0]
    c, s, pl = eng.run_forward_ft(imgs, spds, cmds, 2, 2, 0.0, 0)
    eng.run_backward(pl, torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"), data_only=True)
    with pytest.raises(RuntimeError, match="there is no image gradient"):
        eng.run_input_grads(pl, torch.empty_like(imgs), None)
