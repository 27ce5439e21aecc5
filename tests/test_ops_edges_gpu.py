"""Inputs that i.i.d. Gaussians never produce, against float64 references:

  1. BatchNorm statistics of channels whose mean is far from zero (csrc/bn_pool.hip takes the
     variance as s2/M - mean^2 from fp32 partial sums): the unchanged parity tolerances up to twice
     the largest |mean|/std the network's own BatchNorm inputs reach (R_net, oracle/bn_input_ratio.py;
     DESIGN.md section 3), an error cap that follows from the scheme beyond that;
  2. dead channels (y == 0, rstd = 1/sqrt(eps));
  3. the dropout hash as a random number generator (keep rate, independence between rows, columns,
     sites and seeds), against a numpy restatement of the documented hash;
  4. cilrs_loss_fwd_bwd called directly: batches past one 256-thread trip, sign(0), grad_scale,
     NULL gradient outputs.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- BatchNorm through the C-ABI and in float64 ------------------------------------------------------
def hip_bn(y, gamma, beta, rm, rv, resid, relu, dz, bf16=False):
    """cilrs_bn_train_fwd + cilrs_bn_bwd (bf16: cilrs_bn16_*; y / resid / dz are then bf16 tensors);
    CPU tensors in, a dict of CPU tensors out"""
    L = _L()
    lib = L.lib()
    M, Cc = y.shape
    T = BF16 if bf16 else torch.float32
    yd, dzd = y.cuda(), dz.cuda()
    rd = None if resid is None else resid.cuda()
    gd, bd, rmd, rvd = gamma.cuda(), beta.cuda(), rm.clone().cuda(), rv.clone().cuda()
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stats = torch.full((4 * Cc,), float("nan"), device="cuda")
    part = torch.empty(lib.cilrs_bn_partial_floats(Cc), device="cuda")
    z = torch.full((M, Cc), float("nan"), dtype=T, device="cuda")
    dy = torch.full((M, Cc), float("nan"), dtype=T, device="cuda")
    gout = torch.full((M, Cc), float("nan"), dtype=T, device="cuda")
    dgamma, dbeta = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    coef = torch.empty(3 * Cc, device="cuda")
    if bf16:
        L.check(lib.cilrs_bn16_train_fwd(L.ptr(yd), M, Cc, L.ptr(gd), L.ptr(bd), L.ptr(rmd), L.ptr(rvd),
                                         L.ptr(nbt), 0.1, EPS, L.ptr(rd), relu, L.ptr(stats),
                                         L.ptr(part), L.ptr(z), 0, stream()))
        L.check(lib.cilrs_bn16_bwd(L.ptr(dzd), L.ptr(z), L.ptr(yd), M, Cc, L.ptr(gd), L.ptr(stats), relu,
                                   L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), L.ptr(part), L.ptr(dy),
                                   L.ptr(gout), 0, stream()))
    else:
        L.check(lib.cilrs_bn_train_fwd(L.ptr(yd), M, Cc, L.ptr(gd), L.ptr(bd), L.ptr(rmd), L.ptr(rvd),
                                       L.ptr(nbt), 0.1, EPS, L.ptr(rd), relu, L.ptr(stats), L.ptr(part),
                                       L.ptr(z), stream()))
        L.check(lib.cilrs_bn_bwd(L.ptr(dzd), L.ptr(z), L.ptr(yd), M, Cc, L.ptr(gd), L.ptr(stats), relu,
                                 L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), L.ptr(part), L.ptr(dy),
                                 L.ptr(gout), stream()))
    torch.cuda.synchronize()
    assert int(nbt) == 1
    return {"z": z.cpu().double(), "rm": rmd.cpu().double(), "rv": rvd.cpu().double(),
            "dy": dy.cpu().double(), "dgamma": dgamma.cpu().double(), "dbeta": dbeta.cpu().double(),
            "stats": stats.cpu().double()}


def ref_bn(y, gamma, beta, rm, rv, resid, relu, dz):
    """torch double on the CPU: F.batch_norm and autograd, of the values the kernel was given"""
    M, Cc = y.shape
    yv = y.double().requires_grad_(True)
    gp, bp = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    out = F.batch_norm(yv.view(M, Cc, 1, 1), rm64, rv64, gp, bp, True, 0.1, EPS).view(M, Cc)
    if resid is not None:
        out = out + resid.double()
    if relu:
        out = F.relu(out)
    out.backward(dz.double())
    return {"z": out.detach(), "rm": rm64, "rv": rv64, "dy": yv.grad, "dgamma": gp.grad,
            "dbeta": bp.grad}


def _bn_params(Cc, g):
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g) - 0.5
    rm, rv = torch.rand(Cc, generator=g) - 0.5, torch.rand(Cc, generator=g) + 0.5
    return gamma, beta, rm, rv


# ---- 1. statistics away from zero mean ------------------------------------------------------------------
# oracle/bn_input_ratio.py on the golden train forward: the largest per-channel |mean|/std over the
# inputs of all 36 BatchNorm layers is R_net = 5.20 (visual_encoder.4.2.bn1, channel 60)
R_NET_CEIL = 6
HALF_BF16 = 2.0 ** -8          # half a bf16 spacing relative to the value, at most (test_ops_gpu.py)


def _off_mean_input(M, Cc, sigma, r, g, bf16):
    sign = torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
    y = torch.randn(M, Cc, generator=g) * sigma + r * sigma * sign
    dz = torch.randn(M, Cc, generator=g)
    return (y.to(BF16), dz.to(BF16)) if bf16 else (y, dz)


def _elementwise(got, ref, tol, rel):
    """the bound |got - ref| <= tol + rel * |ref| per element: (largest |got - ref|, largest error as a
    fraction of its bound -- the bound holds when that is <= 1)"""
    err = (got - ref).abs()
    return float(err.max()), float((err / (tol + rel * ref.abs())).max())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M", [3300, 21])
@pytest.mark.parametrize("sigma", [1.0, 0.05])
@pytest.mark.parametrize("r", [0, R_NET_CEIL, 2 * R_NET_CEIL])
def test_bn_off_mean_within_the_networks_range(r, sigma, M, bf16):
    """y = randn * sigma + r * sigma * (+-1 per channel), r up to twice the network's own largest
    ratio, against float64 with the tolerances of test_bn_train_fwd_bwd: 2e-5 max(1, |out|max) for
    z, 5e-5 scale for dy / dgamma / dbeta, 1e-6 / 1e-5 (x max(1, |value|)) for the running statistics.
    The bf16 kernels round z and dy once on the way out: half a bf16 spacing, 2^-8 |ref|, is added
    per element for those two (as in test_bn16_fwd_bwd_on_bf16_tensors); the reference is computed from
    the bf16 values the kernel read."""
    Cc = 64
    g = torch.Generator().manual_seed(1000 * r + M + int(100 * sigma))
    y, dz = _off_mean_input(M, Cc, sigma, r, g, bf16)
    gamma, beta, rm, rv = _bn_params(Cc, g)
    ref = ref_bn(y, gamma, beta, rm, rv, None, 0, dz)
    got = hip_bn(y, gamma, beta, rm, rv, None, 0, dz, bf16)
    rel = HALF_BF16 if bf16 else 0.0
    ez, fz = _elementwise(got["z"], ref["z"], 2e-5 * max(1.0, float(ref["z"].abs().max())), rel)
    edy, fdy = _elementwise(got["dy"], ref["dy"], 5e-5 * max(1.0, float(ref["dy"].abs().max())), rel)
    eg = float((got["dgamma"] - ref["dgamma"]).abs().max())
    eb = float((got["dbeta"] - ref["dbeta"]).abs().max())
    erm = float(((got["rm"] - ref["rm"]).abs() / ref["rm"].abs().clamp_min(1.0)).max())
    erv = float(((got["rv"] - ref["rv"]).abs() / ref["rv"].abs().clamp_min(1.0)).max())
    print(f"BN-EDGE near {'bf16' if bf16 else 'fp32'} M={M} sigma={sigma} r={r}: z {ez:.3e} "
          f"(|z|max {float(ref['z'].abs().max()):.2f}) dy {edy:.3e} (|dy|max "
          f"{float(ref['dy'].abs().max()):.2f}) dgamma {eg:.3e} dbeta {eb:.3e} rm {erm:.3e} rv {erv:.3e}"
          f"; z, dy as fractions of their bounds {fz:.3f} {fdy:.3f}")
    assert fz <= 1.0 and fdy <= 1.0
    assert eg <= 5e-5 * max(1.0, float(ref["dgamma"].abs().max()))
    assert eb <= 5e-5 * max(1.0, float(ref["dbeta"].abs().max()))
    assert erm <= 1e-6 and erv <= 1e-5


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M", [3300, 21])
@pytest.mark.parametrize("sigma", [1.0, 0.05])
@pytest.mark.parametrize("r", [10, 100, 1000])
def test_bn_off_mean_far_from_the_networks_range(r, sigma, M, bf16):
    """Far outside the network's range the scheme's own error shows: an fp32 sum of squares carries
    a relative error of a few units of 2^-24 on mean^2 + std^2, i.e. (1 + r^2) times that on the
    variance, and half of the variance's relative error reaches the normalised output.  Cap:
    2^-22 (1 + r^2) max|zhat| on top of the base tolerance (4-7 x over a CPU emulation of the scheme
    with 64-row partials) -- it catches a reduction that got worse, it is no claim of torch parity.
    gamma = 1, beta = 0, so that z IS the normalised value.  Everything finite, running_var >= 0."""
    Cc = 64
    g = torch.Generator().manual_seed(7000 + r + M + int(100 * sigma))
    y, dz = _off_mean_input(M, Cc, sigma, r, g, bf16)
    _, _, rm, rv = _bn_params(Cc, g)
    gamma, beta = torch.ones(Cc), torch.zeros(Cc)
    got = hip_bn(y, gamma, beta, rm, rv, None, 0, dz, bf16)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    assert bool((got["rv"] >= 0).all())
    y64 = y.double()
    zhat = (y64 - y64.mean(0)) / torch.sqrt(y64.var(0, unbiased=False) + EPS)
    zmax = float(zhat.abs().max())
    cap = 2.0 ** -22 * (1 + r * r) * zmax + 2e-5 * max(1.0, zmax)
    ez, fz = _elementwise(got["z"], zhat, cap, HALF_BF16 if bf16 else 0.0)
    print(f"BN-EDGE far {'bf16' if bf16 else 'fp32'} M={M} sigma={sigma} r={r}: z err {ez:.3e} "
          f"(|zhat|max {zmax:.2f}, cap {cap:.3e}), as a fraction of its bound {fz:.3f}")
    assert fz <= 1.0


# ---- 2. dead channels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3300, 21])
@pytest.mark.parametrize("relu,res", [(0, False), (1, False), (0, True), (1, True)])
def test_bn_dead_channels(M, relu, res):
    """y == 0 in every fourth channel: mean = var = 0, rstd = 1/sqrt(eps) = 316.  There z is beta
    (+ residual, then ReLU) exactly, the running statistics are 0.9 x old, and dy / dgamma / dbeta
    match float64 within the tolerances of test_bn_train_fwd_bwd, dy's scaled by gamma/sqrt(eps) (the
    factor every dy of such a channel carries)."""
    Cc = 64
    g = torch.Generator().manual_seed(40 + M + 2 * relu + int(res))
    y, dz = torch.randn(M, Cc, generator=g), torch.randn(M, Cc, generator=g)
    dead = torch.arange(Cc) % 4 == 1
    y[:, dead] = 0.0
    gamma, beta, rm, rv = _bn_params(Cc, g)
    resid = torch.randn(M, Cc, generator=g) if res else None
    ref = ref_bn(y, gamma, beta, rm, rv, resid, relu, dz)
    got = hip_bn(y, gamma, beta, rm, rv, resid, relu, dz)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    want_z = beta.view(1, Cc).expand(M, Cc)
    if res:
        want_z = want_z + resid                                  # (one fp32 addition, like the kernel's)
    if relu:
        want_z = F.relu(want_z)
    assert torch.equal(got["z"][:, dead].float(), want_z[:, dead]), "dead channels: z != beta (+ res)"
    assert float((got["rm"][dead] - 0.9 * rm[dead].double()).abs().max()) <= 1e-7
    assert float((got["rv"][dead] - 0.9 * rv[dead].double()).abs().max()) <= 1e-7
    tol_dy = 5e-5 * gamma.double()[dead] / math.sqrt(EPS)
    edy = (got["dy"][:, dead] - ref["dy"][:, dead]).abs().max(0).values
    assert bool((edy <= tol_dy).all()), (edy / tol_dy).max()
    assert float(ref["dy"][:, dead].abs().max()) > 100          # (the reference really carries 1/sqrt(eps))
    eg = (got["dgamma"][dead] - ref["dgamma"][dead]).abs().max()
    eb = (got["dbeta"][dead] - ref["dbeta"][dead]).abs().max()
    assert float(eg) <= 5e-5 * max(1.0, float(ref["dgamma"].abs().max()))
    assert float(eb) <= 5e-5 * max(1.0, float(ref["dbeta"].abs().max()))
    # the live channels next to them are not disturbed
    live = ~dead
    ez = (got["z"][:, live] - ref["z"][:, live]).abs().max()
    assert float(ez) <= 2e-5 * max(1.0, float(ref["z"].abs().max()))
    print(f"BN-EDGE dead M={M} relu={relu} res={int(res)}: dy err / tol {float((edy / tol_dy).max()):.3e} "
          f"dgamma {float(eg):.3e} dbeta {float(eb):.3e} live z {float(ez):.3e}")


# ---- 3. the dropout hash ---------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def np_hash_u(seed, site, n):
    """include/cilrs_hip.h, cilrs_dropout: u = top 24 bits of splitmix64's finaliser over
    seed * 0x2545F4914F6CDD1D + (site << 40) + index, as an fp32 in [0, 1); keep where u >= p"""
    base = (seed * 0x2545F4914F6CDD1D + (site << 40)) & M64
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(base)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    r = (x >> np.uint64(32)).astype(np.uint32)
    return (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def np_keep(seed, site, rows, cols, p):
    return (np_hash_u(seed, site, rows * cols) >= np.float32(p)).reshape(rows, cols)


def z_bonferroni(m, z_single=5.0):
    """the z at which m two-sided tests together are as likely to raise a false alarm as ONE test at
    z_single sigma: erfc(z / sqrt 2) = erfc(z_single / sqrt 2) / m  (bisection)"""
    target = math.erfc(z_single / math.sqrt(2.0)) / m
    lo, hi = z_single, z_single + 10.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > target else (lo, mid)
    return hi


DROP_ROWS, DROP_COLS, DROP_LD = 128, 512, 516
DROP_SEED = 0x1234_5678_9ABC
PAD = 7.25


def hip_dropout_mask(rows, cols, ld, p, seed, site):
    """cilrs_dropout on ones inside a pitched matrix; returns the [rows, cols] result (CPU) after
    checking that the pad columns are untouched"""
    L = _L()
    a = torch.full((rows, ld), PAD, device="cuda")
    a[:, :cols] = 1.0
    L.check(L.lib().cilrs_dropout(L.ptr(a), rows, cols, ld, p, seed, site, stream()))
    torch.cuda.synchronize()
    a = a.cpu()
    assert bool((a[:, cols:] == PAD).all()), "pad columns written"
    return a[:, :cols].contiguous()


def mask_statistics(keep, p):
    """the assertions on one [rows, cols] keep mask, shared by the CPU restatement and the kernel:
    overall keep rate within 5 sigma, per-row and per-column rates within z_bonf sigma of their own n
    (Bonferroni factor = rows + cols = 640 tests per mask: z = 6.13 instead of 5)"""
    rows, cols = keep.shape
    n, q = keep.size, 1.0 - float(np.float32(p))
    assert abs(keep.mean() - q) <= 5.0 * math.sqrt(q * (1 - q) / n), ("keep rate", keep.mean(), q)
    z = z_bonferroni(rows + cols)
    assert 6.1 < z < 6.3
    assert np.abs(keep.mean(1) - q).max() <= z * math.sqrt(q * (1 - q) / cols), "a row's keep rate"
    assert np.abs(keep.mean(0) - q).max() <= z * math.sqrt(q * (1 - q) / rows), "a column's keep rate"


def agreement(a, b, p):
    """two independent masks agree on p^2 + (1-p)^2 of the positions, within 5 sigma"""
    pf = float(np.float32(p))
    q = pf * pf + (1 - pf) * (1 - pf)
    frac = float((a == b).mean())
    assert abs(frac - q) <= 5.0 * math.sqrt(q * (1 - q) / a.size), ("agreement", frac, q)


SITE_PAIRS = [(0, 1), (1, 2), (8, 9)]
SEED_STEPS = [1, 1 << 32]


@pytest.mark.parametrize("p", [0.5, 0.1, 0.9])
def test_dropout_hash_statistics(p):
    """The chosen seeds pass every statistic on the numpy restatement (checked right here, on the CPU
    side of this test), and the kernel's masks ARE the restatement's bit for bit -- so a failure
    means the kernel differs from its documented hash."""
    pf = np.float32(p)
    inv = np.float32(1.0) / (np.float32(1.0) - pf)               # 1.0f / (1.0f - p)
    masks = {}
    for site in sorted({s for pair in SITE_PAIRS for s in pair}):
        masks[(DROP_SEED, site)] = np_keep(DROP_SEED, site, DROP_ROWS, DROP_COLS, p)
    for step in SEED_STEPS:
        masks[(DROP_SEED + step, 0)] = np_keep(DROP_SEED + step, 0, DROP_ROWS, DROP_COLS, p)
    for (seed, site), want in masks.items():
        mask_statistics(want, p)                                  # the restatement itself
        got = hip_dropout_mask(DROP_ROWS, DROP_COLS, DROP_LD, p, seed, site).numpy()
        keep = got != 0
        assert np.array_equal(got[keep].view(np.uint32),
                              np.full(int(keep.sum()), inv).view(np.uint32)), "kept value != 1/(1-p)"
        assert np.array_equal(keep, want), f"kernel mask != documented hash (seed {seed:#x} site {site})"
        mask_statistics(keep, p)
        masks[(seed, site)] = keep
    for s0, s1 in SITE_PAIRS:
        agreement(masks[(DROP_SEED, s0)], masks[(DROP_SEED, s1)], p)
    for step in SEED_STEPS:
        agreement(masks[(DROP_SEED, 0)], masks[(DROP_SEED + step, 0)], p)


def test_dropout_mask_does_not_depend_on_the_row_count():
    """index = row * cols + col: rows 0..7 of a (128, 512) call are an (8, 512) call"""
    big = hip_dropout_mask(DROP_ROWS, DROP_COLS, DROP_LD, 0.5, DROP_SEED, 3)
    small = hip_dropout_mask(8, DROP_COLS, DROP_COLS + 4, 0.5, DROP_SEED, 3)
    assert torch.equal(big[:8], small)
    assert torch.equal(small != 0, torch.from_numpy(np_keep(DROP_SEED, 3, 8, DROP_COLS, 0.5)))


def test_dropout_p_zero_is_the_identity():
    L = _L()
    g = torch.Generator().manual_seed(5)
    a = torch.randn(DROP_ROWS, DROP_LD, generator=g)
    ad = a.cuda()
    L.check(L.lib().cilrs_dropout(L.ptr(ad), DROP_ROWS, DROP_COLS, DROP_LD, 0.0, DROP_SEED, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(ad.cpu(), a)                               # values and pad columns alike


# ---- 4. the loss, called directly ------------------------------------------------------------------------------
LOSS_WEIGHTS = [(0.5, 0.45, 0.05, 0.1), (1.0, 1.0, 1.0, 0.0)]


def loss_inputs(B, seed):
    """a third of the control differences exactly zero; brake targets from {0, 1}, as the data has"""
    g = torch.Generator().manual_seed(seed)
    pc, tc = torch.rand(B, 3, generator=g) * 2 - 1, torch.rand(B, 3, generator=g) * 2 - 1
    tc[:, 2] = (torch.rand(B, generator=g) < 0.3).float()
    pc[:, 2] = torch.rand(B, generator=g)
    zero = torch.rand(B, 3, generator=g) < 1.0 / 3.0
    if B >= 3:
        zero.view(-1)[:3] = torch.tensor([True, False, True])    # (both kinds of element in every batch)
    pc[zero] = tc[zero]
    ps, ts = torch.rand(B, generator=g), torch.rand(B, generator=g)
    return pc, tc, ps, ts, zero


def loss_ref64(pc, tc, ps, ts, kind, w, gs):
    """float64, from the fp32 inputs and the fp32 weights the kernel receives"""
    B = pc.shape[0]
    w = [float(np.float32(v)) for v in w]
    d, dsp = pc.double() - tc.double(), ps.double() - ts.double()
    spd = float((dsp * dsp).mean())
    if kind == 0:
        ch = (d * d).mean(0)
        control = float((d * d).mean())
        dpc = 2.0 * d / (3.0 * B) * gs
    else:
        ch = d.abs().mean(0)
        control = w[0] * float(ch[0]) + w[1] * float(ch[1]) + w[2] * float(ch[2])
        dpc = torch.sign(d) * torch.tensor(w[:3], dtype=torch.float64) / B * gs
    out = torch.tensor([control + w[3] * spd, control, float(ch[0]), float(ch[1]), float(ch[2]), spd],
                       dtype=torch.float64)
    return out, dpc, w[3] * 2.0 * dsp / B * gs


def within_ulps(got32, ref64, ulps):
    """|got - ref| <= ulps spacings of fp32 at ref; returns the largest error in spacings"""
    ref32 = np.abs(ref64.numpy()).astype(np.float32)
    spacing = np.spacing(ref32).astype(np.float64)
    err = np.abs(got32.numpy().astype(np.float64) - ref64.numpy()) / spacing
    assert err.max() <= ulps, f"{err.max():.2f} ulp at {np.unravel_index(err.argmax(), err.shape)}"
    return float(err.max())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("weights", LOSS_WEIGHTS)
@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_loss_fwd_bwd_against_float64(kind, B, weights, gs):
    """The six outputs to 1e-6 relative; the gradients to 2 ulp of fp32 (three fp32 operations per
    element after the exact weight products: the difference, the scale by 1/B or 1/(3B), and for the
    speed term the product with the difference); exactly 0 where the difference is 0 (torch's
    sign(0)); with dcontrols NULL, dpred_speed NULL and both NULL the rest is unchanged."""
    L = _L()
    lib = L.lib()
    pc, tc, ps, ts, zero = loss_inputs(B, 900 + B + kind)
    want_out, want_dpc, want_dps = loss_ref64(pc, tc, ps, ts, kind, weights, gs)
    pcd, tcd, psd, tsd = pc.cuda(), tc.cuda(), ps.cuda(), ts.cuda()
    w4 = (C.c_float * 4)(*weights)
    for with_dpc, with_dps in [(True, True), (False, True), (True, False), (False, False)]:
        out = torch.full((6,), float("nan"), device="cuda")
        dpc = torch.full((B, 3), float("nan"), device="cuda") if with_dpc else None
        dps = torch.full((B,), float("nan"), device="cuda") if with_dps else None
        L.check(lib.cilrs_loss_fwd_bwd(L.ptr(pcd), L.ptr(tcd), L.ptr(psd), L.ptr(tsd), B, kind, w4, gs,
                                       L.ptr(dpc), L.ptr(dps), L.ptr(out), stream()))
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all())
        assert bool(((got - want_out).abs() <= 1e-6 * want_out.abs()).all()), (got, want_out)
        if with_dpc:
            gd = dpc.cpu()
            assert bool((gd[zero] == 0).all()), "gradient at a zero difference"
            u = within_ulps(gd, want_dpc, 2)
        if with_dps:
            v = within_ulps(dps.cpu(), want_dps, 2)
    print(f"LOSS kind={kind} B={B} w={weights} gs={gs}: dcontrols {u:.2f} ulp, dpred_speed {v:.2f} ulp")
