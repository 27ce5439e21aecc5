"""SmoothGrad and integrated gradients on the device: the three kernels of csrc/attribution.hip
(cilrs_attr_samples, cilrs_attr_accumulate, cilrs_attr_finalize) and Predictor.attribution on top
of them.

Gates:
  samples, integrated    torch.equal to the fp32 restatement (tests/test_attribution_host.py)
  samples, SmoothGrad    sigma255 = 0: torch.equal to oracle.preprocess_frame; sigma255 = 25: against
                         the float64 evaluation of the same formula from the same hash bits, error
                         <= max(4x the numpy float32 evaluation's, one fp32 ulp of the largest output)
  chunks                 samples 2+2+1 torch.equal to 5 at once; the gradient sum likewise
  accumulate             torch.equal to the sequential fp32 loop
  finalize               attr / signed_map torch.equal to the fp32 expressions; total within
                         (ceil(3HW / threads) + 16) * 2^-24 * sum|attr| of the float64 sum
  Predictor.attribution  samples=1, sigma=0 is Predictor.saliency (np.array_equal); heat, peak (and
                         signed) against the float64 oracle on the same samples: relative L2 error
                         <= max(4x the fp32 CPU oracle's own error, 5e-3) -- the gate of
                         tests/test_saliency_gpu.py; the completeness gap delta within
                         max(4x the fp32 CPU oracle's, 5e-3 |F(x) - F(x0)|) of the float64 oracle's
Every op-level output is pre-filled with NaN inside the guard bands of tests/_guards.py.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cilrs_oracle as O
from _guards import Inputs, guarded
from test_attribution_host import INTEGRATED, SMOOTHGRAD, samples_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5), (2, 7, 33), (1, 88, 200), (2, 8, 12)]     # (B, H, W); the last: 16-byte paths at B = 2
IMG_STD = (0.229, 0.224, 0.225)
SCALE3 = [1.0 / (255.0 * s) for s in IMG_STD]
NAN = float("nan")


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)


def _run_samples(f_dev, b_dev, mode, S, s_begin, s_count, sigma255, seed):
    """cilrs_attr_samples into a NaN-filled guarded buffer; returns the CPU result"""
    L = _lib()
    B, H, W, _ = f_dev.shape
    out, check = guarded(B * s_count * 3 * H * W, name="samples out")
    ins = Inputs(frames=f_dev, baseline=b_dev)
    L.check(L.lib().cilrs_attr_samples(L.ptr(f_dev), L.ptr(b_dev), B, H, W, mode, S, s_begin,
                                       s_count, sigma255, seed, L.ptr(out), stream()))
    check()
    ins.check()
    got = out.view(B * s_count, 3, H, W).cpu()
    assert torch.isfinite(got).all()                            # every element written
    return got


def _chunks(total, sizes):
    s0 = 0
    for n in sizes:
        yield s0, n
        s0 += n
    assert s0 == total


def _frame_major(parts, B):
    """chunks [B*n_i,3,H,W] -> [B*sum n_i,3,H,W] with each frame's samples adjacent"""
    per = [p.view(B, -1, *p.shape[1:]) for p in parts]
    return torch.cat(per, dim=1).reshape(-1, *parts[0].shape[1:])


# ---- 1. cilrs_attr_samples ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("with_baseline", [False, True])
def test_samples_integrated_is_the_fp32_restatement(B, H, W, with_baseline):
    S = 5
    f = _frames(B, H, W, 1 + H)
    base = _frames(B, H, W, 2 + W) if with_baseline else None
    f_dev, b_dev = f.cuda(), base.cuda() if with_baseline else None
    # the torch fp32 restatement, operation by operation
    c = f.float().unsqueeze(1)
    c0 = base.float().unsqueeze(1) if with_baseline else torch.zeros_like(c)
    alpha = (torch.arange(S, dtype=torch.float32) + torch.tensor(0.5)) / torch.tensor(float(S))
    v = c0 + alpha.view(1, S, 1, 1, 1) * (c - c0)
    want = (v / torch.tensor(255.0) - torch.tensor(O.IMG_MEAN)) / torch.tensor(O.IMG_STD)
    want = want.permute(0, 1, 4, 2, 3).reshape(B * S, 3, H, W).contiguous()
    assert torch.equal(want, torch.from_numpy(samples_ref(
        f.numpy(), base.numpy() if with_baseline else None, INTEGRATED, S, 0, S, 0.0, 0)))
    got = _run_samples(f_dev, b_dev, INTEGRATED, S, 0, S, 0.0, 0)
    assert torch.equal(got, want)
    parts = [_run_samples(f_dev, b_dev, INTEGRATED, S, s0, n, 0.0, 0) for s0, n in _chunks(S, (2, 2, 1))]
    assert torch.equal(_frame_major(parts, B), want)


def test_samples_integrated_at_the_frame_is_the_preprocessing():
    """A path point at the frame itself is the frame's preprocessing bit for bit.  No midpoint has
    alpha = 1, so the path is made to end where it starts: with the frame as its own baseline
    every v = c0 + alpha * (c - c0) is c."""
    f = O.synthetic_batch(2, seed=9)[4]
    want = torch.cat([O.preprocess_frame(x) for x in f])
    f_dev = torch.from_numpy(f).cuda()
    got = _run_samples(f_dev, f_dev.clone(), INTEGRATED, 3, 0, 3, 0.0, 0)
    for b in range(2):
        for j in range(3):
            assert torch.equal(got[b * 3 + j], want[b])


def test_samples_smoothgrad_without_noise_is_preprocess_frame():
    f = O.synthetic_batch(2, seed=5)[4]
    want = torch.cat([O.preprocess_frame(x) for x in f])
    got = _run_samples(torch.from_numpy(f).cuda(), None, SMOOTHGRAD, 3, 0, 3, 0.0, 11)
    for b in range(2):
        for j in range(3):
            assert torch.equal(got[b * 3 + j], want[b])


@pytest.mark.parametrize("B,H,W,S,s_begin,s_count",
                         [(b, h, w, 5, 0, 5) for b, h, w in SHAPES] +
                         [(1, 88, 200, 1 << 20, (1 << 20) - 2, 2)])     # the counter passes 2^32
def test_samples_smoothgrad_noise_against_float64(B, H, W, S, s_begin, s_count):
    sigma255, seed = 25.0, 0x1234567890ABCDEF
    f = _frames(B, H, W, 3 + H)
    got = _run_samples(f.cuda(), None, SMOOTHGRAD, S, s_begin, s_count, sigma255, seed).double()
    f64 = torch.from_numpy(samples_ref(f.numpy(), None, SMOOTHGRAD, S, s_begin, s_count, sigma255,
                                       seed, np.float64))
    f32 = torch.from_numpy(samples_ref(f.numpy(), None, SMOOTHGRAD, S, s_begin, s_count, sigma255,
                                       seed, np.float32)).double()
    e_gpu, e_np = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    ulp = float(np.spacing(np.float32(float(f64.abs().max()))))
    print(f"[{B},{H},{W}] S={S} from {s_begin}: max error vs float64: kernel {e_gpu:.3e}, numpy "
          f"float32 {e_np:.3e} (one ulp of the largest output {ulp:.3e})")
    assert e_gpu <= max(4.0 * e_np, ulp)
    # the noise is there: standard deviation sigma255 / (255 * std_c) per channel
    if H * W >= 1000:
        clean = torch.from_numpy(samples_ref(f.numpy(), None, SMOOTHGRAD, S, s_begin, s_count, 0.0,
                                             seed, np.float64))
        sd = (got - clean).std(dim=(0, 2, 3))
        want_sd = torch.tensor([sigma255 / (255.0 * s) for s in IMG_STD], dtype=torch.float64)
        assert float(((sd - want_sd).abs() / want_sd).max()) <= 0.05


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_samples_smoothgrad_chunks_are_slices_of_the_whole(B, H, W):
    f_dev = _frames(B, H, W, 4 + H).cuda()
    whole = _run_samples(f_dev, None, SMOOTHGRAD, 5, 0, 5, 25.0, 77)
    parts = [_run_samples(f_dev, None, SMOOTHGRAD, 5, s0, n, 25.0, 77) for s0, n in _chunks(5, (2, 2, 1))]
    assert torch.equal(_frame_major(parts, B), whole)
    other = _run_samples(f_dev, None, SMOOTHGRAD, 5, 0, 5, 25.0, 78)
    assert not torch.equal(other, whole)                        # another seed, other noise
    v = whole.view(B, 5, 3, H, W)
    assert not torch.equal(v[:, 0], v[:, 1])                    # and every sample its own


def test_samples_from_unaligned_tensors_are_the_same():
    """H * W is a multiple of 4 but the tensors are not 16-byte (frames: 4-byte) aligned: the
    one-pixel-per-thread kernel serves them, with the same result"""
    L = _lib()
    B, H, W, S = 2, 8, 12, 3
    f = _frames(B, H, W, 21)
    want = _run_samples(f.cuda(), None, SMOOTHGRAD, S, 0, S, 25.0, 3)
    raw = torch.zeros(f.numel() + 1, dtype=torch.uint8, device="cuda")
    raw[1:].copy_(f.flatten())
    n = B * S * 3 * H * W
    out, check = guarded(n + 1, name="samples out (+4 bytes)")
    L.check(L.lib().cilrs_attr_samples(C.c_void_p(raw.data_ptr() + 1), None, B, H, W, SMOOTHGRAD, S,
                                       0, S, 25.0, 3, C.c_void_p(out.data_ptr() + 4), stream()))
    check()
    assert torch.equal(out[1:].view(B * S, 3, H, W).cpu(), want)
    assert bool(torch.isnan(out[:1]).all())


# ---- 2. cilrs_attr_accumulate -------------------------------------------------------------------------
def _run_accumulate(g_dev, B, n, H, W, first, acc):
    L = _lib()
    L.check(L.lib().cilrs_attr_accumulate(L.ptr(g_dev), *g_dev.stride(), B, n, H, W, first,
                                          L.ptr(acc), stream()))


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("channels_last", [False, True])
def test_accumulate_is_the_sequential_fp32_loop(B, H, W, channels_last):
    S = 5
    gen = torch.Generator().manual_seed(B * 1000 + H * W)
    g = torch.randn(B * S, 3, H, W, generator=gen) * torch.logspace(-3, 3, B * S).view(-1, 1, 1, 1)
    want = torch.zeros(B, 3, H, W)
    for j in range(S):
        want = want + g.view(B, S, 3, H, W)[:, j]
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    g_dev = g.cuda().contiguous(memory_format=fmt)
    ins = Inputs(dimage=g_dev)
    # one chunk of 5, `first` over garbage (NaN) in acc
    acc, check = guarded(B * 3 * H * W, name="acc")
    _run_accumulate(g_dev, B, S, H, W, 1, acc)
    check()
    one = acc.view(B, 3, H, W).cpu()
    assert torch.equal(one, want)
    # 2 + 2 + 1: chunks of a frame-major batch are not slices of it, so each is gathered
    acc2, check2 = guarded(B * 3 * H * W, name="acc (chunks)")
    for s0, n in _chunks(S, (2, 2, 1)):
        part = g.view(B, S, 3, H, W)[:, s0:s0 + n].reshape(B * n, 3, H, W)
        part = part.cuda().contiguous(memory_format=fmt)
        _run_accumulate(part, B, n, H, W, 1 if s0 == 0 else 0, acc2)
    check2()
    ins.check()
    assert torch.equal(acc2.view(B, 3, H, W).cpu(), want)
    # first = 0 continues from what acc holds
    acc3, check3 = guarded(B * 3 * H * W, fill=None, name="acc (continued)")
    start = torch.randn(B, 3, H, W, generator=gen)
    acc3.copy_(start.flatten())
    _run_accumulate(g_dev, B, S, H, W, 0, acc3)
    check3()
    cont = start.clone()
    for j in range(S):
        cont = cont + g.view(B, S, 3, H, W)[:, j]
    assert torch.equal(acc3.view(B, 3, H, W).cpu(), cont)


# ---- 3. cilrs_attr_finalize ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("mode,with_baseline", [(SMOOTHGRAD, False), (INTEGRATED, False),
                                                (INTEGRATED, True)])
def test_finalize_is_the_fp32_expression(B, H, W, mode, with_baseline):
    L = _lib()
    S = 5
    threads = L.lib().cilrs_attr_finalize_threads()
    gen = torch.Generator().manual_seed(B + H * W + mode)
    acc = torch.randn(B, 3, H, W, generator=gen) * 3.0
    f = _frames(B, H, W, 5 + H)
    base = _frames(B, H, W, 6 + W) if with_baseline else None
    inv_s = torch.tensor(1.0) / torch.tensor(float(S))
    want = acc * inv_s
    if mode == INTEGRATED:
        diff = f.int() - (base.int() if with_baseline else 0)
        scale = torch.tensor(SCALE3, dtype=torch.float32).view(1, 3, 1, 1)
        want = want * (diff.float().permute(0, 3, 1, 2) * scale)
    want_signed = (want[:, 0] + want[:, 1]) + want[:, 2]
    acc_dev, f_dev = acc.cuda(), f.cuda()
    b_dev = base.cuda() if with_baseline else None
    cs = (C.c_float * 3)(*SCALE3)
    ins = Inputs(acc=acc_dev, frames=f_dev, baseline=b_dev)
    outs = []
    for _ in range(2):
        attr, c1 = guarded(B * 3 * H * W, name="attr")
        signed, c2 = guarded(B * H * W, name="signed_map")
        total, c3 = guarded(B, name="total")
        L.check(L.lib().cilrs_attr_finalize(
            L.ptr(acc_dev), L.ptr(f_dev) if mode == INTEGRATED else None, L.ptr(b_dev), B, H, W, mode,
            S, cs if mode == INTEGRATED else None, L.ptr(attr), L.ptr(signed), L.ptr(total), stream()))
        c1(), c2(), c3()
        outs.append((attr.view(B, 3, H, W).cpu(), signed.view(B, H, W).cpu(), total.cpu()))
    ins.check()
    attr, signed, total = outs[0]
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)                                # bit-identical on a second call
    assert torch.equal(attr, want)
    assert torch.equal(signed, want_signed)
    t64 = want.double().sum((1, 2, 3))
    bound = (math.ceil(3 * H * W / threads) + 16) * 2.0 ** -24 * want.double().abs().sum((1, 2, 3))
    err = (total.double() - t64).abs()
    print(f"[{B},{H},{W}] mode {mode}: |total - float64 sum| {err.tolist()} (bound {bound.tolist()})")
    assert bool((err <= bound).all())
    # signed_map and total are optional
    attr2, c1 = guarded(B * 3 * H * W, name="attr (alone)")
    L.check(L.lib().cilrs_attr_finalize(
        L.ptr(acc_dev), L.ptr(f_dev) if mode == INTEGRATED else None, L.ptr(b_dev), B, H, W, mode, S,
        cs if mode == INTEGRATED else None, L.ptr(attr2), None, None, stream()))
    c1()
    assert torch.equal(attr2.view(B, 3, H, W).cpu(), want)


# ---- 4. refusals ----------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_write_nothing():
    L = _lib()
    lib = L.lib()
    B, H, W, S = 2, 7, 33, 5
    f_dev = _frames(B, H, W, 1).cuda()
    out, check_out = guarded(B * S * 3 * H * W, name="samples out")
    g_dev = torch.randn(B * S, 3, H, W, device="cuda")
    acc, check_acc = guarded(B * 3 * H * W, name="acc")
    attr, check_attr = guarded(B * 3 * H * W, name="attr")
    total, check_total = guarded(B, name="total")
    cs = (C.c_float * 3)(*SCALE3)
    fp, op, gp, ap, tp = L.ptr(f_dev), L.ptr(out), L.ptr(g_dev), L.ptr(acc), L.ptr(attr)
    st = g_dev.stride()

    def refused(rc, what):
        assert rc != 0, what
        msg = lib.cilrs_last_error()
        assert msg and what.encode() in msg, (what, msg)

    smp = lib.cilrs_attr_samples
    refused(smp(None, None, B, H, W, SMOOTHGRAD, S, 0, S, 1.0, 0, op, stream()), "NULL")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 0, S, 1.0, 0, None, stream()), "NULL")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, 0, 0, 1, 1.0, 0, op, stream()), "at least 1")
    refused(smp(fp, None, B, H, W, INTEGRATED, -4, 0, 1, 1.0, 0, op, stream()), "at least 1")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, -1, 2, 1.0, 0, op, stream()), "outside")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 4, 2, 1.0, 0, op, stream()), "outside")
    refused(smp(fp, None, B, H, W, INTEGRATED, S, S, 1, 1.0, 0, op, stream()), "outside")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 0, 0, 1.0, 0, op, stream()), "outside")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 0, S, -1.0, 0, op, stream()), "sigma255")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 0, S, float("nan"), 0, op, stream()), "sigma255")
    refused(smp(fp, None, B, H, W, SMOOTHGRAD, S, 0, S, float("inf"), 0, op, stream()), "sigma255")
    refused(smp(fp, None, 1 << 20, 1024, 1024, SMOOTHGRAD, 1 << 30, 0, 1, 1.0, 0, op, stream()), "2^63")
    refused(smp(fp, None, B, H, W, 2, S, 0, S, 1.0, 0, op, stream()), "mode")
    accf = lib.cilrs_attr_accumulate
    refused(accf(None, *st, B, S, H, W, 1, ap, stream()), "NULL")
    refused(accf(gp, *st, B, S, H, W, 1, None, stream()), "NULL")
    refused(accf(gp, st[0], st[1], -st[2], st[3], B, S, H, W, 1, ap, stream()), "negative stride")
    refused(accf(gp, *st, B, 0, H, W, 1, ap, stream()), "bad shape")
    fin = lib.cilrs_attr_finalize
    refused(fin(None, fp, None, B, H, W, INTEGRATED, S, cs, tp, None, L.ptr(total), stream()), "NULL")
    refused(fin(ap, fp, None, B, H, W, INTEGRATED, S, cs, None, None, L.ptr(total), stream()), "NULL")
    refused(fin(ap, fp, None, B, H, W, INTEGRATED, 0, cs, tp, None, L.ptr(total), stream()), "at least 1")
    refused(fin(ap, None, None, B, H, W, INTEGRATED, S, cs, tp, None, L.ptr(total), stream()), "need the frames")
    refused(fin(ap, fp, None, B, H, W, INTEGRATED, S, None, tp, None, L.ptr(total), stream()), "need the frames")
    refused(fin(ap, fp, None, B, H, W, 7, S, cs, tp, None, L.ptr(total), stream()), "mode")
    for chk, buf in ((check_out, out), (check_acc, acc), (check_attr, attr), (check_total, total)):
        chk()
        assert bool(torch.isnan(buf).all())                     # nothing was written


# ---- 5. Predictor.attribution ---------------------------------------------------------------------------
OUTPUT_W = {"steer": (1.0, 0.0, 0.0, 0.0), "speed": (0.0, 0.0, 0.0, 1.0)}
H88, W200 = 88, 200


def make_model(seed=0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def oracles():
    return {torch.float64: O.build_oracle(0).double().eval(), torch.float32: O.build_oracle(0).eval()}


def _rel(a, ref):
    return float((a.double() - ref.double()).norm()) / max(float(ref.double().norm()), 1e-30)


def _oracle_grads(orc, x, speeds_kmh, commands, weights, per_frame, dtype):
    """d (w . (controls, pred_speed)) / d x of the eval-mode oracle for samples x [B*n,3,H,W]
    (frame-major), and F = w . outputs per sample"""
    x = x.detach().clone().to(dtype).requires_grad_()
    spd = torch.tensor([min(s / O.SPEED_NORM, 1.0) for s in speeds_kmh], dtype=dtype)
    cmd = torch.tensor(commands, dtype=torch.long)
    pc, ps = orc(x, spd.repeat_interleave(per_frame), cmd.repeat_interleave(per_frame))
    w = torch.tensor(weights, dtype=dtype)
    f = (pc * w[:3]).sum(1) + ps.reshape(-1) * w[3]
    f.sum().backward()
    return x.grad, f.detach()


def _device_samples(u8, base, mode, S, sigma255, seed):
    """the call's own samples, from the same kernel with the same seed: bit-identical by contract"""
    f_dev = torch.from_numpy(u8).cuda()
    b_dev = torch.from_numpy(base).cuda() if base is not None else None
    return _run_samples(f_dev, b_dev, mode, S, 0, S, sigma255, seed)


@pytest.mark.parametrize("B", [1, 2])
def test_attribution_of_one_clean_sample_is_saliency(B):
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(B, seed=40 + B)[4]
    speeds, cmds = [12.0, 55.0][:B], [2, 0][:B]
    pr = Predictor(make_model(), batch=B)
    for output in ("steer", (0.5, 0.0, -1.0, 2.0)):
        want = pr.saliency(u8, speeds, cmds, output=output)
        out, heat, peak, info = pr.attribution(u8, speeds, cmds, output=output, method="smoothgrad",
                                               samples=1, sigma=0)
        assert info["method"] == "smoothgrad" and info["samples"] == 1
        assert np.array_equal(out, want[0])
        assert np.array_equal(heat, want[1])
        assert np.array_equal(peak, want[2])
        assert float(peak.min()) > 0 and float(heat.max()) == 1.0


@pytest.mark.parametrize("B", [1, 2])
def test_smoothgrad_vs_oracle(B, oracles):
    from cilrs_mi355.predict import Predictor
    S, chunk, sigma, seed = 4, 2, 0.1, 5
    u8 = O.synthetic_batch(B, seed=50 + B)[4]
    speeds, cmds = [12.0, 55.0][:B], [2, 0][:B]
    pr = Predictor(make_model(), batch=B)
    pb = pr.predict_batch(u8, speeds, cmds)
    out, heat, peak, info = pr.attribution(u8, speeds, cmds, output="steer", method="smoothgrad",
                                           samples=S, sigma=sigma, seed=seed, chunk=chunk)
    assert info == dict(method="smoothgrad", samples=S, chunk=chunk)
    assert out.shape == (B, 4) and out.dtype == np.float32
    assert heat.shape == (B, H88, W200) and heat.dtype == np.float32 and peak.shape == (B,)
    x = _device_samples(u8, None, SMOOTHGRAD, S, 255.0 * sigma, seed)
    ref = {}
    for dt in (torch.float64, torch.float32):
        g, _ = _oracle_grads(oracles[dt], x, speeds, cmds, OUTPUT_W["steer"], S, dt)
        mean = g.view(B, S, 3, H88, W200).sum(1) / S
        scale = torch.tensor(SCALE3, dtype=dt).view(1, 3, 1, 1)
        s = (mean.abs() * scale).amax(1)
        pk = s.amax((1, 2))
        ref[dt] = (s / pk.view(-1, 1, 1), pk)
    h64, p64 = ref[torch.float64]
    h32, p32 = ref[torch.float32]
    e_gpu, e_cpu = _rel(torch.from_numpy(heat), h64), _rel(h32, h64)
    pe_gpu = float(((torch.from_numpy(peak).double() - p64).abs() / p64).max())
    pe_cpu = float(((p32.double() - p64).abs() / p64).max())
    print(f"smoothgrad B={B}: heat relative L2 vs float64 {e_gpu:.3e} (fp32 CPU oracle {e_cpu:.3e}); "
          f"peak relative error {pe_gpu:.3e} (CPU {pe_cpu:.3e})")
    assert (peak > 0).all() and float(heat.max()) == 1.0 and float(heat.min()) >= 0.0
    assert e_gpu <= max(4.0 * e_cpu, 5e-3)
    assert pe_gpu <= max(4.0 * pe_cpu, 5e-3)
    assert np.abs(out[:, :3] - pb[:, :3]).max() <= 1e-4
    assert np.abs(out[:, 3] - pb[:, 3]).max() <= 90e-4


@pytest.mark.parametrize("with_baseline", [False, True])
def test_integrated_gradients_vs_oracle(with_baseline, oracles):
    from cilrs_mi355.predict import Predictor
    S, output = 4, "steer"
    u8 = O.synthetic_batch(1, seed=61)[4]
    base = O.synthetic_batch(1, seed=62)[4] if with_baseline else None
    speeds, cmds = [30.0], [1]
    x = _device_samples(u8, base, INTEGRATED, S, 0.0, 0)
    x_end = torch.cat([O.preprocess_frame(f) for f in u8])
    x_0 = torch.cat([O.preprocess_frame(f) for f in (base if with_baseline else np.zeros_like(u8))])
    ref = {}
    for dt in (torch.float64, torch.float32):
        g, _ = _oracle_grads(oracles[dt], x, speeds, cmds, OUTPUT_W[output], S, dt)
        _, f_ends = _oracle_grads(oracles[dt], torch.cat([x_end, x_0]), speeds, cmds, OUTPUT_W[output],
                                  2, dt)
        attr = (g.sum(0, keepdim=True) / S) * (x_end.to(dt) - x_0.to(dt))
        s = attr.abs().amax(1)
        pk = s.amax((1, 2))
        total = attr.sum((1, 2, 3))
        ref[dt] = dict(heat=s / pk.view(-1, 1, 1), peak=pk, signed=attr.sum(1), total=total,
                       gap=float(f_ends[0] - f_ends[1]),
                       delta=float(total[0] - (f_ends[0] - f_ends[1])))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    pr = Predictor(make_model())
    for chunk in (4, 3):                        # 3: a short last chunk on a plan of its own
        out, heat, peak, info = pr.attribution(u8, speeds, cmds, output=output, method="integrated",
                                               samples=S, baseline=base, chunk=chunk)
        assert info["method"] == "integrated" and info["samples"] == S and info["chunk"] == chunk
        assert info["signed"].shape == (1, H88, W200) and info["total"].shape == (1,)
        assert info["baseline_out"].shape == (1,) and info["delta"].shape == (1,)
        tag = f"integrated baseline={'u8' if with_baseline else 'black'} chunk={chunk}"
        for name, got in (("heat", heat), ("signed", info["signed"])):
            e_gpu, e_cpu = _rel(torch.from_numpy(got), r64[name]), _rel(r32[name], r64[name])
            print(f"{tag}: {name} relative L2 vs float64 {e_gpu:.3e} (fp32 CPU oracle {e_cpu:.3e})")
            assert e_gpu <= max(4.0 * e_cpu, 5e-3), (tag, name)
        pe_gpu = abs(float(peak[0]) - float(r64["peak"])) / float(r64["peak"])
        pe_cpu = abs(float(r32["peak"]) - float(r64["peak"])) / float(r64["peak"])
        print(f"{tag}: peak relative error {pe_gpu:.3e} (CPU {pe_cpu:.3e})")
        assert pe_gpu <= max(4.0 * pe_cpu, 5e-3)
        assert float(heat.max()) == 1.0 and float(heat.min()) >= 0.0
        delta = float(info["delta"][0])
        d_gpu, d_cpu = abs(delta - r64["delta"]), abs(r32["delta"] - r64["delta"])
        print(f"{tag}: completeness gap delta {delta:.6e} (float64 oracle {r64['delta']:.6e}, fp32 CPU "
              f"{r32['delta']:.6e}); F(x) - F(x0) = {r64['gap']:.6e}; total {float(info['total'][0]):.6e}")
        assert d_gpu <= max(4.0 * d_cpu, 5e-3 * abs(r64["gap"]))
        # delta is what it says: total - (w . out_raw - baseline_out), raw outputs (speed / 90)
        f_x = float(out[0, 0])                  # output = steer
        assert abs(delta - (float(info["total"][0]) - (f_x - float(info["baseline_out"][0])))) <= 1e-6


def test_attribution_is_reproducible_and_leaves_the_predictor_alone():
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(1, seed=71)[4]
    pr = Predictor(make_model())                # B = 1: the persistent predictor
    assert pr.persistent
    before = pr.predict_batch(u8, [20.0], [3])
    kw = dict(output="throttle", method="smoothgrad", samples=3, sigma=0.1, seed=9, chunk=2)
    a = pr.attribution(u8, [20.0], [3], **kw)
    b = pr.attribution(u8, [20.0], [3], **kw)
    for p, q in zip(a[:3], b[:3]):
        assert np.array_equal(p, q)
    assert a[3] == b[3]
    c = pr.attribution(u8, [20.0], [3], **dict(kw, seed=10))
    assert not np.array_equal(a[1], c[1])       # another seed, another map
    assert np.array_equal(a[0], c[0])           # of the same clean forward
    ig = dict(output="throttle", method="integrated", samples=2)
    d = pr.attribution(u8, [20.0], [3], **ig)
    e = pr.attribution(u8, [20.0], [3], **ig)
    for p, q in zip(d[:3], e[:3]):
        assert np.array_equal(p, q)
    assert sorted(d[3]) == sorted(e[3])
    for k in ("signed", "total", "baseline_out", "delta"):
        assert np.array_equal(d[3][k], e[3][k])
    after = pr.predict_batch(u8, [20.0], [3])
    assert np.array_equal(before, after)        # the persistent single-frame state still serves
    assert pr.persistent and pr.degraded_ticks_left == 0 and pr.barrier_timeouts == 0


def test_attribution_misuse_raises_before_any_launch():
    from cilrs_mi355.predict import Predictor
    u8 = O.synthetic_batch(1, seed=3)[4]
    m = make_model()
    pr = Predictor(m)
    eng = m.engine()
    params, epoch, plans = eng.params.clone(), eng.weights_epoch, len(eng.plans)
    for bad in (dict(method="vargrad"), dict(output="steering"), dict(samples=0), dict(sigma=-0.5),
                dict(sigma=float("nan")), dict(chunk=0),
                dict(method="integrated", baseline=u8[0]),
                dict(method="integrated", baseline=u8.astype(np.float32))):
        with pytest.raises(ValueError):
            pr.attribution(u8, [10.0], [1], **bad)
    with pytest.raises(RuntimeError, match="out of range"):
        pr.attribution(u8, [10.0], [4])
    with pytest.raises(RuntimeError):
        pr.attribution(u8[0], [10.0], [1])                       # not a batch of frames
    with pytest.raises(RuntimeError):
        pr.attribution(u8.astype(np.float32), [10.0], [1])
    with pytest.raises(RuntimeError):
        pr.attribution(u8, [10.0, 20.0], [1])
    cam = np.zeros((1, 600, 800, 4), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="network resolution"):
        pr.attribution(cam, [10.0], [1])                         # no stand-alone device resize
    eng.train_precision = "bf16"
    try:
        with pytest.raises(RuntimeError, match="fp32 plans only"):
            pr.attribution(u8, [10.0], [1])
    finally:
        eng.train_precision = "fp32"
    torch.cuda.synchronize()
    assert torch.equal(eng.params, params) and eng.weights_epoch == epoch
    assert len(eng.plans) == plans and getattr(pr, "_att", None) is None      # nothing was set up
