"""Layer-by-layer walk of the fp32 eval-mode forward -- shared by tests/test_eval32_layers_gpu.py
(the two HIP realisations) and tests/test_eval32_layers_host.py (a CPU backend and sabotaged ones).

walk() goes through the ORACLE's module structure in order -- stem, max-pool, every BasicBlock's
conv1, its downsample where present, its conv2, the heads -- and compares every tensor the
realisation under test STORED with a float64 computation on the tensor it stored one step earlier.
The input of every step is the realisation's own output, so a ReLU decision flipped by rounding
cannot propagate: the only freedom left to a step is the order of its fp32 sums.

A convolution step, flags as trunk_fwd_eval32 and b1_build set them:

    acc64 = conv2d(x.double(), w.double(), stride, pad)
    scale = gamma / sqrt(running_var + 1e-5);  shift = beta - running_mean * scale      (float64)
    ref   = relu_post?( relu?(acc64 * scale + shift) + identity )

    step        relu  identity  relu_post
    stem        yes   no        no
    conv1       yes   no        no
    downsample  no    no        no
    conv2       no    yes       yes

Per tensor, no element left out: finite; |got - ref| <= 2e-5 * max(1, max(|acc64 * scale| + |shift|
+ |identity|)) (the project's fp32 convolution contract, _tol of test_ops_gpu.py, on the magnitude
of the terms that are summed); rms(got - ref) <= R * max(rms(cpu32 - ref), 1e-7 * rms(ref)), cpu32
being torch's fp32 realisation of the same step on the same stored input.  The max-pool is bit-equal
to F.max_pool2d of the stored stem output, x4[..., :3] within 1e-5 of the oracle's normalised image,
x4[..., 3] finite (the stem multiplies it by zero weights), and the four outputs within
2e-5 * max(1, max|ref|) of the oracle's heads run in float64 on the float64 average of the last
stored feature map.

Every failed assertion is collected; WalkFailure is raised at the end and lists the tensors that
failed, so a test can ask for "this tensor and no other".
"""
import copy

import torch
import torch.nn.functional as F

import infer16_emulation as E
from test_infer16_gpu import _conv_numbers, _models  # noqa: F401  (_models: re-exported to the tests)

TOL = 2e-5                 # elementwise, relative to the magnitude of the summed terms
TOL_X4 = 1e-5              # preprocess (tests/test_infer16_gpu.py uses the same)
NOISE_FLOOR = 1e-7         # of rms(ref): below this e_cpu says nothing


class WalkFailure(AssertionError):
    def __init__(self, failures):
        self.failures = failures                      # [(tensor name, what went wrong)]
        super().__init__("; ".join(f"{n}: {m}" for n, m in failures))

    def tensors(self):
        return sorted({n for n, _ in self.failures})


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def fold64(bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + E.BN_EPS)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale


def conv_step64(x, conv, bn, identity, relu, relu_post):
    """(ref, magnitude) of one step in float64 on the stored fp32 input x (NCHW)."""
    scale, shift = fold64(bn)
    acc = F.conv2d(x.double(), conv.weight.detach().double(), None, conv.stride, conv.padding)
    y = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    mag = (acc * scale.view(1, -1, 1, 1)).abs() + shift.abs().view(1, -1, 1, 1)
    if relu:
        y = F.relu(y)
    if identity is not None:
        y = y + identity.double()
        mag = mag + identity.double().abs()
    if relu_post:
        y = F.relu(y)
    return y, float(mag.max())


def conv_step32(x, conv, bn, identity, relu, relu_post, mutate=None):
    """The same step in torch fp32: the yardstick of the noise gate and the host tests' backend.
    mutate(acc) may change the raw convolution result in place (the sabotaged backends)."""
    scale, shift = E.fold_scale_shift(bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                      bn.running_var)
    acc = F.conv2d(x.float(), conv.weight.detach(), None, conv.stride, conv.padding)
    if mutate is not None:
        mutate(acc)
    y = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if relu:
        y = F.relu(y)
    if identity is not None:
        y = y + identity.float()
    if relu_post:
        y = F.relu(y)
    return y


def steps(orc):
    """[(name, conv, bn, input key, identity key, relu, relu_post)] in the walk's order; a key is the
    name of an earlier step ("pool" for the max-pool output)."""
    ve = orc.visual_encoder
    out = [("stem", ve[0], ve[1], "image", None, 1, 0)]
    cur = "pool"
    for bi, blk in enumerate(E.trunk_blocks(orc)):
        main, down = E.block_convs(blk)
        assert len(main) == 2, "BasicBlock networks only"
        n1, nd, n2 = f"block {bi} conv1", f"block {bi} downsample", f"block {bi} conv2"
        out.append((n1, main[0][0], main[0][1], cur, None, 1, 0))
        identity = cur
        if down is not None:
            out.append((nd, down[0], down[1], cur, None, 0, 0))
            identity = nd
        out.append((n2, main[1][0], main[1][1], n1, identity, 0, 1))
        cur = n2
    return out


@torch.no_grad()
def heads64(orc, feat_map, spd, cmd):
    """float64 heads of the oracle on the float64 average of the stored feature map (NCHW):
    [B, 4] = (steer, throttle, brake, raw predicted speed)."""
    o = copy.deepcopy(orc).double()
    visual = E.avgpool(feat_map, torch.float64)
    speed_feat = o.speed_encoder(spd.double().unsqueeze(1))
    combined = torch.cat([visual, speed_feat], dim=1)
    pred_speed = o.speed_predictor(visual).squeeze(1)
    all_out = torch.stack([br(combined) for br in o.control_branches], dim=0)
    idx = cmd.view(1, -1, 1).expand(1, visual.size(0), 3)
    return torch.cat([all_out.gather(0, idx).squeeze(0), pred_speed.unsqueeze(1)], dim=1)


def check_heads(orc, feat_map, spd, cmd, outputs, what, failures=None):
    """The four outputs of the realisation (controls [B,3], raw pred_speed [B]) against heads64."""
    own = failures is None
    failures = [] if own else failures
    ref = heads64(orc, feat_map, spd, cmd)
    got = torch.cat([outputs[0].double().view(-1, 3), outputs[1].double().view(-1, 1)], dim=1)
    bound = TOL * max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max()) if torch.isfinite(got).all() else float("inf")
    print(f"EVAL32 {what} heads cmd {cmd.tolist()}: max err {err:.3e} = {err / bound:.3f} x bound")
    if not err <= bound:
        failures.append(("heads", f"outputs off by {err:.3e} > {bound:.3e}"))
    if own and failures:
        raise WalkFailure(failures)
    return err / bound


@torch.no_grad()
def walk(orc, x4, fetch, cmd, spd, outputs, image=None, R=None, what=""):
    """orc: CPU oracle in eval mode; x4 [B,H,W,4]: the stored fp32 image; fetch(i): stored output
    of convolution i (engine numbering, -1 the max-pool) as an NCHW (or [B,C,H*W]) CPU tensor;
    outputs = (controls [B,3], raw pred_speed [B]) of the realisation for (cmd, spd); image: the
    oracle's normalised image [B,3,H,W] (None: that check is the caller's); R: the noise gate's
    factor (None: ratios are measured and printed, not asserted).
    Returns (rows, last feature map), rows = [dict(name, conv, bound_ratio, e_hip, e_cpu, ratio)];
    raises WalkFailure naming every tensor that failed."""
    assert not orc.training
    failures, rows = [], []
    numbers = _conv_numbers(orc)
    if not torch.isfinite(x4).all():
        failures.append(("x4", "non-finite (the pad channel meets zero weights: 0 * inf = nan)"))
    img_dev = x4[..., :3].permute(0, 3, 1, 2).contiguous()
    if image is not None:
        e = float((img_dev - image).abs().max())
        print(f"EVAL32 {what} x4: max |x4 - normalised image| {e:.3e}")
        if not e <= TOL_X4:
            failures.append(("x4", f"off the oracle's normalised image by {e:.3e}"))
    stored = {"image": img_dev}
    for name, conv, bn, kx, kid, relu, relu_post in steps(orc):
        ci = numbers[id(conv)]
        x = stored[kx]
        identity = None if kid is None else stored[kid]
        ref, mag = conv_step64(x, conv, bn, identity, relu, relu_post)
        c32 = conv_step32(x, conv, bn, identity, relu, relu_post)
        got = fetch(ci)
        assert got.numel() == ref.numel(), f"{name}: {got.numel()} stored values, {ref.numel()} expected"
        got = got.reshape(ref.shape).float()
        stored[name] = got
        bound = TOL * max(1.0, mag)
        e_cpu = rms(c32.double() - ref)
        yard = max(e_cpu, NOISE_FLOOR * rms(ref))
        if not torch.isfinite(got).all():
            failures.append((name, f"{int((~torch.isfinite(got)).sum())} non-finite elements"))
            rows.append(dict(name=name, conv=ci, bound_ratio=float("inf"), e_hip=float("inf"),
                             e_cpu=e_cpu, ratio=float("inf")))
            print(f"EVAL32 {what} {name} (conv {ci}) {tuple(ref.shape)}: NON-FINITE")
            stored[name] = torch.nan_to_num(got, nan=0.0, posinf=0.0, neginf=0.0)
            continue
        err = (got.double() - ref).abs()
        worst, e_hip = float(err.max()) / bound, rms(got.double() - ref)
        ratio = e_hip / yard
        rows.append(dict(name=name, conv=ci, bound_ratio=worst, e_hip=e_hip, e_cpu=e_cpu, ratio=ratio))
        print(f"EVAL32 {what} {name} (conv {ci}) {tuple(x.shape)} -> {tuple(ref.shape)}: max err "
              f"{float(err.max()):.3e} = {worst:.4f} x bound; e_hip {e_hip:.3e} e_cpu {e_cpu:.3e} "
              f"e_hip/e_cpu {ratio:.3f}")
        nbad = int((err > bound).sum())
        if nbad:
            at = [int(v) for v in (err == err.max()).nonzero()[0]]
            failures.append((name, f"{nbad}/{ref.numel()} elements beyond {bound:.3e} (worst "
                                   f"{worst:.1f} x bound at {at})"))
        if R is not None and not e_hip <= R * yard:
            failures.append((name, f"rms error {e_hip:.3e} > {R} x {yard:.3e}"))
        if name == "stem":
            pool = fetch(-1)
            want = F.max_pool2d(got, 3, 2, 1)
            assert pool.numel() == want.numel(), "max-pool: stored size"
            pool = pool.reshape(want.shape).float()
            stored["pool"] = pool
            nd = int((pool != want).sum()) if torch.isfinite(pool).all() else pool.numel()
            print(f"EVAL32 {what} max-pool {tuple(want.shape)}: {nd} elements differ")
            if nd:
                failures.append(("max-pool", f"{nd}/{want.numel()} elements differ from "
                                             "F.max_pool2d of the stored stem output"))
                stored["pool"] = torch.nan_to_num(pool, nan=0.0, posinf=0.0, neginf=0.0)
    last = stored[steps(orc)[-1][0]]
    check_heads(orc, last, spd, cmd, outputs, what, failures)
    if failures:
        raise WalkFailure(failures)
    return rows, last


# ---- a CPU realisation of the same contract (the host tests' backend) --------------------------
class CpuBackend:
    """The fp32 eval forward step by step in torch, every tensor kept where fetch() finds it.
    sabotage = None or (kind, step name):
      "tap"    the (kh, kw) = (2, 2) corner tap dropped at output pixel (0, 0) of that 3x3 step;
      "tap1"   the same tap dropped for input channel 0 alone;
      "relu"   that conv2's block applies its ReLU before the residual instead of after it;
      "stale"  the last output pixel of that step keeps the value `previous` (another run's
               tensors) holds there -- what a skipped last row of a ragged tile leaves behind."""

    def __init__(self, orc, image, spd, cmd, sabotage=None, previous=None):
        self.numbers = _conv_numbers(orc)
        B, _, H, W = image.shape
        self.x4 = torch.cat([image.permute(0, 2, 3, 1), torch.zeros(B, H, W, 1)], dim=3).contiguous()
        self.z, self.by_name = {}, {"image": image}
        kind, where = sabotage or (None, None)
        with torch.no_grad():
            for name, conv, bn, kx, kid, relu, relu_post in steps(orc):
                x = self.by_name[kx]
                identity = None if kid is None else self.by_name[kid]
                mutate = None
                if kind in ("tap", "tap1") and name == where:
                    assert conv.kernel_size == (3, 3) and conv.padding == (1, 1)
                    nch = 1 if kind == "tap1" else conv.in_channels

                    def mutate(acc, x=x, conv=conv, nch=nch):
                        # output pixel (0, 0) reads input (kh - 1, kw - 1): tap (2, 2) is input (1, 1)
                        acc[:, :, 0, 0] -= x[:, :nch, 1, 1] @ conv.weight.detach()[:, :nch, 2, 2].t()
                if kind == "relu" and name == where:
                    assert identity is not None
                    y = conv_step32(x, conv, bn, None, 1, 0) + identity
                else:
                    y = conv_step32(x, conv, bn, identity, relu, relu_post, mutate)
                if kind == "stale" and name == where:
                    y[-1, :, -1, -1] = previous.by_name[name][-1, :, -1, -1]
                self.by_name[name] = y
                self.z[self.numbers[id(conv)]] = y
                if name == "stem":
                    self.by_name["pool"] = self.z[-1] = F.max_pool2d(y, 3, 2, 1)
                self.last = y
            out = E.heads(orc, E.avgpool(self.last, torch.float32), spd, cmd)
        self.outputs = (out[0], out[1])

    def fetch(self, i):
        return self.z[i]
