"""Mask-matched float64 gradient oracle of the fp32 backward pass -- shared by
tests/test_masked_grads_gpu.py (the HIP engine) and tests/test_masked_grads_host.py (a CPU backend
and sabotaged ones).

The backward pass depends on decisions the forward took: every ReLU's sign, the tap every stem
pooling window kept, the BatchNorm mode of every layer.  Two runs of the same step that take them
on their own differ on a handful of units whose pre-activation is within rounding of zero, and one
such unit late in the trunk moves every gradient upstream of it by ~1e-3 -- which is why the
unforced gates of tests/test_model_gpu.py stop at 5e-3.  Here the decisions are READ from the
realisation under test (decisions()) and the oracle is forced to take exactly them
(cilrs_oracle.forward_with_decisions): the two backward passes are then the same linear map and
differ by rounding alone.

check(backend, case, R):
  1. float64 oracle, forced forward + backward from fixed upstream gradients (dcontrols,
     dpred_speed ~ N(0, 1) / B from a seeded generator; no loss: its L1 term carries a sign
     decision of its own and test_loss_fwd_bwd_against_float64 pins it) -> g64, dimage64, dspeed64;
  2. the fp32 CPU oracle, the same forced forward + backward -> cpu32: the reference's arithmetic
     under the same decisions, so e_cpu = its distance from float64 is summation order alone;
  3. consistency of the forced decisions, in the float64 run (ConsistencyFailure; without it a
     wrong forward would be followed rather than caught):
       * a unit whose mask disagrees with the sign of its own float64 pre-activation has
         |pre-activation| <= 1e-5, and there are at most max(64, 2e-5 * numel) of them per ReLU
         (both numbers: test_relu_decisions_at_b128_differ_only_at_rounding_level);
       * the tap every pooling window was told to keep holds a value within 1e-5 of the window's
         maximum -- of relu(BatchNorm output), what the reference pools --, and stem_on agrees
         with the sign of the kept BatchNorm output under the same two rules;
       * the forced float64 outputs agree with the backend's within TOL_OUT;
  4. the gates, for every parameter tensor of the trainable range (+ dimage, dspeed where the case
     asks), no percentile, no flip branch, no element left out:
       ||got - g64|| <= R * max(||cpu32 - g64||, 2.5e-7 * ||g64||)
       max|got - g64| <= R * max(max|cpu32 - g64|, 2.5e-7 * max|g64|)
       every element finite;  ||got - g64|| <= 1e-4 * ||g64|| whatever R is (CAP)
     every failure is collected, GradFailure names the tensors;
  5. returns the worst ratios (R = None: measured and printed, only finiteness and CAP asserted).
"""
import copy

import torch
import torch.nn.functional as F

import cilrs_oracle as O

TOL_OUT = 1e-4          # outputs (tests/test_model_gpu.py)
PRE_TOL = 1e-5          # a decision may disagree with float64 only on a pre-activation this small
FLOOR = 2.5e-7          # few-ulp floor of e_cpu (_grad_budget_check)
CAP = 1e-4              # relative-L2 error no tensor may exceed, 10x below one flipped decision
N_CHILDREN = {0: 0, 1: 4, 2: 5, 3: 6, 4: 7, 5: 8}     # visual_encoder[:n] = the first e groups
HEAD_WHICH = {"s1": 0, "s2": 1, "p1": 2, "p2": 3, "h1": 4, "h2": 5}   # cilrs_net_head_activation_info


class GradFailure(AssertionError):
    def __init__(self, failures):
        self.failures = failures                      # [(tensor name, what went wrong)]
        super().__init__("; ".join(f"{n}: {m}" for n, m in failures))

    def tensors(self):
        return sorted({n for n, _ in self.failures})


class ConsistencyFailure(GradFailure):
    """Step 3: the decisions handed over are not the ones of this forward."""


# ---- cases ---------------------------------------------------------------------------------------
def case(name, mode="train", trunk="resnet34", B=8, H=88, W=200, seed=10, nc=4, e=0, inputs=False,
         env=None):
    """mode "train" | "frozen" | "ft" (eval-mode prefix of e groups, backward stops there);
    inputs: dimage and dspeed too; env: library switches of a child process."""
    return dict(name=name, mode=mode, trunk=trunk, B=B, H=H, W=W, seed=seed, nc=nc, e=e,
                inputs=inputs, env=env or {})


def build_oracle(c):
    """The fp32 CPU oracle of the case, portable weights (running statistics off 0 / 1)."""
    if c["trunk"] == "resnet50":
        import resnet50_oracle as R50
        m = R50.CILRSResNet50Oracle(c["nc"], 0.0)
    else:
        m = O.CILRSOracle(c["nc"], 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    return m


def inputs_of(c):
    """(image, speed, command) on the CPU; every command gets the same share of the rows."""
    img, spd, cmd = O.synthetic_batch(c["B"], c["seed"], c["H"], c["W"])[:3]
    if c["nc"] != 4:
        cmd = torch.arange(c["B"]) % c["nc"]
    return img, spd, cmd


def upstream_of(c):
    g = torch.Generator().manual_seed(7000 + c["seed"])
    return (torch.randn(c["B"], 3, generator=g) / c["B"], torch.randn(c["B"], generator=g) / c["B"])


def bn_batch_of(orc, c):
    """Per convolution: BatchNorm on the batch statistics?"""
    return {ci: c["mode"] == "train" or (c["mode"] == "ft" and grp >= c["e"])
            for ci, grp, _, _, _ in O.trunk_convs(orc)}


def trainable_of(orc, c):
    frozen = tuple(f"visual_encoder.{i}." for i in range(N_CHILDREN[c["e"] if c["mode"] == "ft" else 0]))
    return [n for n, _ in orc.named_parameters() if not (frozen and n.startswith(frozen))]


def head_keys(orc):
    return ["s1", "s2", "p1", "p2"] + [f"h{l}.{k}" for k in range(len(orc.control_branches))
                                       for l in (1, 2)]


# ---- the record ----------------------------------------------------------------------------------
def decisions(backend):
    """What the backend's forward decided, read from what it stored: mask = z > 0 of every
    convolution that ends in a ReLU, the stem's argmax, stem_on = max-pool output > 0, the head
    masks."""
    orc = backend.orc
    relu = {ci: backend.z(ci) > 0 for ci, _, _, _, ends in O.trunk_convs(orc) if ends and ci > 0}
    for key in head_keys(orc):
        relu[key] = backend.head(key) > 0
    return dict(relu=relu, stem_argmax=backend.stem_argmax(), stem_on=backend.z(-1) > 0,
                bn_batch=bn_batch_of(orc, backend.case))


def forced_run(orc, dtype, img, spd, cmd, dec, dc, dp, names, want_inputs, taps=None):
    """Forced forward + backward in `dtype`: (controls, pred_speed, {name: gradient})."""
    m = copy.deepcopy(orc).to(dtype)
    params = dict(m.named_parameters())
    for n, p in params.items():
        p.requires_grad_(n in names)
    x = img.to(dtype).clone().requires_grad_(want_inputs)
    s = spd.to(dtype).clone().requires_grad_(want_inputs)
    f = O.ForcedDecisions(dec["relu"], dec["stem_argmax"], dec["stem_on"], dec["bn_batch"], taps)
    c, ps = O.forward_with_decisions(m, x, s, cmd, f)
    ins = [params[n] for n in names] + ([x, s] if want_inputs else [])
    keys = list(names) + (["dimage", "dspeed"] if want_inputs else [])
    gs = torch.autograd.grad([c, ps], ins, [dc.to(dtype), dp.to(dtype)])
    return c.detach(), ps.detach(), {k: g.detach().double() for k, g in zip(keys, gs)}


def consistency(dec, taps, out64, outputs, what=""):
    """Step 3 on the float64 run's pre-activations; [(name, message)]."""
    fails = []

    def sign_rule(name, mask, pre):
        bad = mask != (pre > 0)
        n = int(bad.sum())
        if not n:
            return 0, 0.0
        mag = float(pre[bad].abs().max())
        if not mag <= PRE_TOL:
            fails.append((name, f"{int((bad & (pre.abs() > PRE_TOL)).sum())} units decided against "
                                f"a float64 pre-activation of up to {mag:.3e}"))
        if n > max(64, int(2e-5 * pre.numel())):
            fails.append((name, f"{n} of {pre.numel()} units decided against float64"))
        return n, mag

    tot, worst = 0, 0.0
    for key, mask in dec["relu"].items():
        n, mag = sign_rule(f"relu {key}", mask, taps[key])
        tot, worst = tot + n, max(worst, mag)
    z = taps["stem"]
    kept = O.pool_gather(z, dec["stem_argmax"])
    short = F.max_pool2d(F.relu(z), 3, 2, 1) - F.relu(kept)
    if not float(short.max()) <= PRE_TOL:
        fails.append(("stem argmax", f"{int((short > PRE_TOL).sum())} windows kept a tap up to "
                                     f"{float(short.max()):.3e} below the window's maximum"))
    n, mag = sign_rule("stem_on", dec["stem_on"], kept)
    print(f"MASKED {what} decisions: {tot + n} units decided against float64 (largest "
          f"pre-activation {max(worst, mag):.2e}); worst pooling shortfall {float(short.max()):.2e}")
    got = torch.cat([outputs[0].double().view(-1, 3), outputs[1].double().view(-1, 1)], dim=1)
    ref = torch.cat([out64[0].view(-1, 3), out64[1].view(-1, 1)], dim=1)
    err = float((got - ref).abs().max()) if torch.isfinite(got).all() else float("inf")
    if not err <= TOL_OUT:
        fails.append(("outputs", f"forced float64 outputs differ from the backend's by {err:.3e}"))
    return fails


def check(backend, c, R=None):
    """See the module docstring.  Returns dict(l2=worst L2 ratio, elem=worst element ratio,
    rel=worst relative-L2 error of the backend, rows=[per tensor])."""
    orc, what = backend.orc, c["name"]
    img, spd, cmd = backend.image, backend.speed, backend.command
    dc, dp = upstream_of(c)
    names = trainable_of(orc, c)
    try:
        dec = decisions(backend)
        O.pool_index(dec["stem_argmax"], *_stem_hw(c))
    except ValueError as exc:
        raise ConsistencyFailure([("stem argmax", str(exc))])
    taps = {}
    c64, s64, g64 = forced_run(orc, torch.float64, img, spd, cmd, dec, dc, dp, names, c["inputs"],
                               taps)
    fails = consistency(dec, taps, (c64, s64), backend.outputs, what)
    if fails:
        raise ConsistencyFailure(fails)
    del taps
    _, _, g32 = forced_run(orc, torch.float32, img, spd, cmd, dec, dc, dp, names, c["inputs"])
    got = backend.backward(dc, dp, c["inputs"])
    fails, rows = [], []
    for k, ref in g64.items():
        g = got[k].double().reshape(ref.shape)
        if not torch.isfinite(g).all():
            fails.append((k, f"{int((~torch.isfinite(g)).sum())} non-finite elements"))
            rows.append(dict(name=k, l2=float("inf"), elem=float("inf"), rel=float("inf")))
            continue
        nrm, mx = float(ref.norm()), float(ref.abs().max())
        e_hip, e_cpu = float((g - ref).norm()), float((g32[k] - ref).norm())
        m_hip, m_cpu = float((g - ref).abs().max()), float((g32[k] - ref).abs().max())
        yard, myard = max(e_cpu, FLOOR * nrm), max(m_cpu, FLOOR * mx)
        l2 = e_hip / yard if yard > 0 else (0.0 if e_hip == 0 else float("inf"))
        el = m_hip / myard if myard > 0 else (0.0 if m_hip == 0 else float("inf"))
        rel = e_hip / nrm if nrm > 0 else (0.0 if e_hip == 0 else float("inf"))
        rows.append(dict(name=k, l2=l2, elem=el, rel=rel, e_cpu=e_cpu / nrm if nrm > 0 else 0.0))
        if R is not None and not l2 <= R:
            fails.append((k, f"L2 error {e_hip:.3e} > {R} x {yard:.3e}"))
        if R is not None and not el <= R:
            fails.append((k, f"element error {m_hip:.3e} > {R} x {myard:.3e}"))
        if not rel <= CAP:
            fails.append((k, f"relative L2 error {rel:.3e} above the cap {CAP:.0e}"))
    w = {key: max(rows, key=lambda r: r[key]) for key in ("l2", "elem", "rel")}
    print(f"MASKED {what}: {len(rows)} tensors; worst L2 ratio {w['l2']['l2']:.3f} ({w['l2']['name']}), "
          f"worst element ratio {w['elem']['elem']:.3f} ({w['elem']['name']}), worst relative L2 "
          f"error {w['rel']['rel']:.3e} ({w['rel']['name']})")
    if fails:
        raise GradFailure(fails)
    return dict(l2=w["l2"]["l2"], elem=w["elem"]["elem"], rel=w["rel"]["rel"], rows=rows)


def _stem_hw(c):
    return (c["H"] + 6 - 7) // 2 + 1, (c["W"] + 6 - 7) // 2 + 1


@torch.no_grad()
def check_caps(backend, c):
    """Step 3 alone (no backward): raises ConsistencyFailure."""
    dec = decisions(backend)
    taps = {}
    f = O.ForcedDecisions(dec["relu"], dec["stem_argmax"], dec["stem_on"], dec["bn_batch"], taps)
    m = copy.deepcopy(backend.orc).double()
    out = O.forward_with_decisions(m, backend.image.double(), backend.speed.double(),
                                   backend.command, f)
    fails = consistency(dec, taps, out, backend.outputs, c["name"])
    if fails:
        raise ConsistencyFailure(fails)


# The smallest cases that reach each backward kernel family (tests/test_masked_grads_gpu.py runs
# them on the engine; tests/test_masked_grads_host.py checks on the CPU that their inputs keep an
# fp32 realisation inside every cap of step 3).  seed 10: the golden batch of step_cfg*_b8.json.
GPU_CASES = [
    case("train_b8"),
    case("train_b3_odd", B=3, H=90, W=202, seed=31),
    case("train_b1", B=1, seed=32),
    case("train_b32", B=32, seed=777),
    case("train_b8_wino", env={"CILRS_WINO": "2"}),
    case("train_b8_wino_serial", env={"CILRS_WINO": "2", "CILRS_OVERLAP": "0"}),
    case("frozen_b4", mode="frozen", B=4, seed=33, inputs=True),
    case("ft3_b8", mode="ft", e=3),
    case("resnet50_b4", trunk="resnet50", B=4, H=64, W=64, seed=34),
    case("nc6_b12", nc=6, B=12, H=64, W=64, seed=35),
    case("resnet50_b3_odd", trunk="resnet50", B=3, H=90, W=202, seed=36),
]


# ---- a CPU realisation of the same contract (the host tests' backend) ----------------------------
class _Natural(O.ForcedDecisions):
    """forward_with_decisions taking every decision itself (relu, max_pool2d) and keeping what the
    engine keeps: z per convolution, the max-pool output and argmax, the head activations."""

    def __init__(self, bn_batch):
        super().__init__(None, None, None, bn_batch)
        self.kept = {}

    def relu(self, key, x):
        y = F.relu(x)
        self.kept[key] = y.detach().contiguous()
        return y

    def stem(self, z):
        pool, idx = F.max_pool2d(F.relu(z), 3, 2, 1, return_indices=True)
        ho, wo = pool.shape[2:]
        row, col = idx // z.size(3), idx % z.size(3)
        kh = row - (torch.arange(ho).view(1, 1, ho, 1) * 2 - 1)
        kw = col - (torch.arange(wo).view(1, 1, 1, wo) * 2 - 1)
        self.kept["argmax"] = (kh * 3 + kw).to(torch.uint8)
        self.kept[-1] = pool.detach().contiguous()
        return pool


class _MaskBwd(torch.autograd.Function):
    """x * m_fwd whose backward multiplies by m_bwd: a mask that went stale between the passes."""

    @staticmethod
    def forward(ctx, x, m_fwd, m_bwd):
        ctx.save_for_backward(m_bwd)
        return x * m_fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class _GatherBwd(torch.autograd.Function):
    """pool_gather(z, a_fwd) whose backward scatters to the taps a_bwd."""

    @staticmethod
    def forward(ctx, z, a_fwd, a_bwd):
        ctx.save_for_backward(O.pool_index(a_bwd, z.size(2), z.size(3)))
        ctx.shape = z.shape
        return O.pool_gather(z, a_fwd)

    @staticmethod
    def backward(ctx, g):
        dz = g.new_zeros(ctx.shape).flatten(2).scatter_add_(2, ctx.saved_tensors[0], g.flatten(2))
        return dz.view(ctx.shape), None, None


class _Sabotaged(O.ForcedDecisions):
    """ForcedDecisions with backward-only deviations: relu_bwd {key: mask the backward uses},
    argmax_bwd: the taps the stem's backward scatters to."""

    def __init__(self, dec, relu_bwd=None, argmax_bwd=None):
        super().__init__(dec["relu"], dec["stem_argmax"], dec["stem_on"], dec["bn_batch"])
        self.relu_bwd, self.argmax_bwd = relu_bwd or {}, argmax_bwd

    def relu(self, key, x):
        if key in self.relu_bwd:
            return _MaskBwd.apply(x, self.relu_masks[key].to(x.dtype), self.relu_bwd[key].to(x.dtype))
        return super().relu(key, x)

    def stem(self, z):
        if self.argmax_bwd is None:
            return super().stem(z)
        return _GatherBwd.apply(z, self.stem_argmax, self.argmax_bwd) * self.stem_on.to(z.dtype)


class CpuBackend:
    """The fp32 oracle on a channels_last image (another summation order than step 2's run on a
    contiguous one) in place of the engine: it takes its own decisions in the forward, stores the
    tensors the accessors expose, and computes its gradients from what it stored.
    sabotage = None or (kind, argument):
      ("tap", name)        tap (kh, kw) = (1, 2) of the 3x3 weight gradient `name` zeroed;
      ("dbeta", name)      the BatchNorm bias gradient `name` scaled by 1 + 1e-3;
      ("stale", conv)      the backward of that convolution's ReLU reads a mask that is wrong on
                           0.1 % of its units (at least 4);
      ("pool", None)       one window's tap moved to a neighbour in the backward only;
      ("head", "h1.<k>")   the most active column of that branch's first mask dropped in the
                           backward only;
      ("sign", conv)       the STORED z of that convolution has the wrong sign on 1 % of its units."""

    def __init__(self, c, sabotage=None):
        self.case, self.orc = c, build_oracle(c)
        self.image, self.speed, self.command = inputs_of(c)
        self.sabotage = sabotage or (None, None)
        self.f = _Natural(bn_batch_of(self.orc, c))
        with torch.no_grad():
            out = O.forward_with_decisions(self.orc, self._image_cl(), self.speed, self.command, self.f)
        self.outputs = (out[0], out[1])

    def _image_cl(self):
        return self.image.contiguous(memory_format=torch.channels_last)

    def _some_units(self, numel, frac, seed):
        n = max(4, int(frac * numel))
        return torch.randperm(numel, generator=torch.Generator().manual_seed(seed))[:n]

    def z(self, ci):
        z = self.f.kept[ci]
        kind, arg = self.sabotage
        if kind == "sign" and ci == arg:
            z = z.clone()
            at = self._some_units(z.numel(), 0.01, 5)
            flat = z.view(-1)
            flat[at] = torch.where(flat[at] > 0, torch.zeros(()), torch.ones(()))
        return z

    def head(self, key):
        return self.f.kept[key]

    def stem_argmax(self):
        return self.f.kept["argmax"]

    def backward(self, dc, dp, want_inputs):
        kind, arg = self.sabotage
        clean = copy.copy(self)
        clean.sabotage = (None, None)
        dec = decisions(clean)
        relu_bwd, argmax_bwd = {}, None
        if kind == "stale":
            m = dec["relu"][arg].clone()
            at = self._some_units(m.numel(), 1e-3, 6)
            m.view(-1)[at] = ~m.view(-1)[at]
            relu_bwd[arg] = m
        elif kind == "head":
            m = dec["relu"][arg].clone()
            rows = self.command == int(arg.split(".")[1])          # the rows this branch serves
            col = int(m[rows].sum(0).argmax())
            assert m[rows][:, col].any()
            m[:, col] = False
            relu_bwd[arg] = m
        elif kind == "pool":
            a = dec["stem_argmax"].clone()
            b, ch, oh, ow = 0, 5, a.size(2) // 2, a.size(3) // 2
            while not dec["stem_on"][b, ch, oh, ow]:
                ow += 1
            a[b, ch, oh, ow] = (int(a[b, ch, oh, ow]) + 1) % 9
            argmax_bwd = a
        names = trainable_of(self.orc, self.case)
        params = dict(self.orc.named_parameters())
        for n, p in params.items():
            p.requires_grad_(n in names)
        x = self._image_cl().clone().requires_grad_(want_inputs)
        s = self.speed.clone().requires_grad_(want_inputs)
        out = O.forward_with_decisions(self.orc, x, s, self.command,
                                       _Sabotaged(dec, relu_bwd, argmax_bwd))
        ins = [params[n] for n in names] + ([x, s] if want_inputs else [])
        keys = list(names) + (["dimage", "dspeed"] if want_inputs else [])
        got = {k: g.detach().clone() for k, g in zip(keys, torch.autograd.grad(list(out), ins, [dc, dp]))}
        if kind == "tap":
            assert got[arg].shape[2:] == (3, 3)
            got[arg][:, :, 1, 2] = 0
        elif kind == "dbeta":
            got[arg] *= 1 + 1e-3
        return got


# ---- the HIP engine ------------------------------------------------------------------------------
class EngineBackend:
    """Engine.run_forward / run_forward_frozen / run_forward_ft with dropout 0, then run_backward
    (+ run_input_grads); every stored tensor read through the C-ABI's test accessors."""

    def __init__(self, c):
        import ctypes as C
        from cilrs_mi355 import CILRS, CILRSResNet50
        from cilrs_mi355 import _lib as L
        self.C, self.L = C, L
        self.case, self.orc = c, build_oracle(c)
        self.image, self.speed, self.command = inputs_of(c)
        m = (CILRSResNet50 if c["trunk"] == "resnet50" else CILRS)(c["nc"], 0.0)
        m.load_state_dict(self.orc.state_dict(), strict=True)
        self.model = m.cuda()
        self.eng = eng = self.model.engine()
        dev = [t.cuda() for t in (self.image, self.speed, self.command)]
        if c["mode"] == "train":
            self.model.train()
            ctl, ps, self.pl = eng.run_forward(*dev, True, 0.0, 0)
        elif c["mode"] == "frozen":
            self.model.eval()
            ctl, ps, self.pl = eng.run_forward_frozen(*dev)
        else:
            self.model.train()
            ctl, ps, self.pl = eng.run_forward_ft(*dev, c["e"], c["e"], 0.0, 0)
        torch.cuda.synchronize()
        self.pl.check_status()
        self.outputs = (ctl.cpu(), ps.cpu())

    def wino_convs(self):
        return self.pl.wino_convs()

    def z(self, ci):
        C, L = self.C, self.L
        yo, zo, n, ch = L.sz(), L.sz(), L.sz(), L.i32()
        L.check(L.lib().cilrs_net_activation_info(self.pl.handle, ci, C.byref(yo), C.byref(zo),
                                                  C.byref(n), C.byref(ch)))
        ws = self.pl.workspace.view(torch.float32)
        z = ws[zo.value:zo.value + n.value].view(self.pl.batch, -1, ch.value).permute(0, 2, 1)
        hw = z.size(2)
        shape = next(s for s in self._maps() if s[0] * s[1] == hw)
        return z.contiguous().cpu().view(self.pl.batch, ch.value, *shape)

    def _maps(self):
        """(h, w) of the stem output, the max-pool output and the four layers."""
        h, w = _stem_hw(self.case)
        out = [(h, w)]
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((h, w))
        for _ in range(3):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out.append((h, w))
        return out

    def head(self, key):
        C, L = self.C, self.L
        name, _, k = key.partition(".")
        off, rows, cols, ld = L.sz(), L.i32(), L.i32(), L.i32()
        L.check(L.lib().cilrs_net_head_activation_info(self.pl.handle, HEAD_WHICH[name], int(k or 0),
                                                       C.byref(off), C.byref(rows), C.byref(cols),
                                                       C.byref(ld)))
        ws = self.pl.workspace.view(torch.float32)
        a = ws[off.value:off.value + (rows.value - 1) * ld.value + cols.value]
        return torch.as_strided(a, (rows.value, cols.value), (ld.value, 1)).cpu()

    def stem_argmax(self):
        """The stored argmax; behind an eval-mode prefix (no argmax is written there) the taps of
        the stem output the prefix stored, first of equal values as the kernels take it."""
        ho, wo = self._maps()[1]
        if self.case["mode"] == "ft" and self.case["e"] > 0:
            f = _Natural({})
            f.stem(self.z(0))
            return f.kept["argmax"]
        C, L = self.C, self.L
        off, n = L.sz(), L.sz()
        L.check(L.lib().cilrs_net_pool_argmax_info(self.pl.handle, C.byref(off), C.byref(n)))
        assert n.value == self.pl.batch * ho * wo * 64
        a = self.pl.workspace[off.value:off.value + n.value].view(self.pl.batch, ho, wo, 64)
        return a.permute(0, 3, 1, 2).contiguous().cpu()

    def backward(self, dc, dp, want_inputs):
        eng, pl = self.eng, self.pl
        eng.grads.zero_()
        eng.run_backward(pl, dc.cuda().contiguous(), dp.cuda().contiguous())
        got = {}
        if want_inputs:
            dimage = torch.empty(pl.batch, 3, pl.h, pl.w, device=eng.device)
            dspeed = torch.empty(pl.batch, device=eng.device)
            eng.run_input_grads(pl, dimage, dspeed)
            got["dimage"], got["dspeed"] = dimage.cpu(), dspeed.cpu()
        torch.cuda.synchronize()
        for (n, _, _, _), g in zip(eng.params_layout, eng.grad_views):
            got[n] = g.detach().cpu().clone()
        return got
