"""Sharpness-aware minimisation on the device: cilrs_sam_perturb / cilrs_sam_restore inside guard
bands against the two CPU statements of tests/_sam.py (float64, and fp32 in the header's operation
order: bit for bit), the identities, determinism and range independence, the refusals; then the
Trainer: one SAM step is the composition of public pieces, off is the parent's step, sam_every, EMA,
data parallel, and Trainer.sharpness.

Bounds (include/cilrs_hip.h "sharpness-aware minimisation").  S: no sequential run of double
additions is longer than 1,024 terms, so S is within 2^-40 relative of the exactly rounded sum
(math.fsum of the float64 squares, which are exact).  norm: one unit in the last place of
math.sqrt(S).  scale: the same double division as Python's, exactly.  The new p: bit for bit the
fp32 statement with s32 = float32(scale); against float64 the rule of _optim.gate.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import _ema as E
import _optim as Q
import _sam as S
import cilrs_oracle as O
from _guards import PATTERN, Inputs, guarded

pytestmark = pytest.mark.gpu

# One workgroup covers one chunk of cilrs_sam_chunk_floats() = 4096 floats in four trips of 256
# threads x 4 floats.  4 and 8: one and two busy lanes; chunk - 4 / chunk / chunk + 4 straddle the
# second workgroup; 3 chunks + 12 has a three-quad tail; 1,048,580 = 256 chunks + 1 quad is the
# smallest size at which a thread of the finalise adds a second chunk sum.
CHUNK = 4096
SIZES = [4, 8, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 12, 1_048_580]
RHOS = [0.0, 0.05, 2.0]
BLOCK = 256                                   # one Gaussian scale per block of 256 elements


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_chunk_constant():
    assert _L().lib().cilrs_sam_chunk_floats() == CHUNK


@functools.lru_cache(maxsize=None)
def make_data(n, seed=0):
    """(p, g) on the CPU: per-block Gaussians whose scales run through 1e-6 .. 1e2, in a different
    phase for p and g; read-only by convention (shared between the tests)"""
    gen = torch.Generator().manual_seed(1000 + seed + n)
    blocks = torch.arange(n) // BLOCK
    p = torch.randn(n, generator=gen) * 10.0 ** ((blocks % 9) - 6).float()
    g = torch.randn(n, generator=gen) * 10.0 ** (((blocks * 4 + 3) % 9) - 6).float()
    return p, g


@functools.lru_cache(maxsize=None)
def reference(n, rho, adaptive):
    """(p64, S, norm, scale) of the float64 statement, once per case"""
    p, g = make_data(n)
    return S.perturb64(p, g, rho, adaptive)


def gbuf(cpu, name):
    v, check = guarded(cpu.numel(), dtype=cpu.dtype, fill=None, guard=4096, name=name)
    v.copy_(cpu)
    return v, check


class Call:
    """One cilrs_sam_perturb inside guard bands: params, grads, backup of exactly n floats, scratch
    of exactly cilrs_sam_scratch_bytes(n) bytes, out3 of exactly three doubles (not the scratch's
    tail: that has to keep its pattern)."""

    def __init__(self, p_cpu, g_cpu):
        L = _L()
        self.n = p_cpu.numel()
        self.p, self.check_p = gbuf(p_cpu, "params")
        self.g, self.check_g = gbuf(g_cpu, "grads")
        self.backup, self.check_b = guarded(self.n, fill=float("nan"), guard=4096, name="backup")
        nbytes = L.lib().cilrs_sam_scratch_bytes(self.n)
        self.nchunks = (self.n + CHUNK - 1) // CHUNK
        assert nbytes == ((self.nchunks + 3) * 8 + 15) // 16 * 16
        self.scratch, self.check_s = guarded(nbytes, dtype=torch.uint8, fill=None, name="scratch")
        self.out3, self.check_o = guarded(3, dtype=torch.float64, fill=float("nan"), name="out3")
        self.const = Inputs(grads=self.g)

    def perturb(self, rho, adaptive):
        L = _L()
        return L.lib().cilrs_sam_perturb(L.ptr(self.p), L.ptr(self.g), L.ptr(self.backup), self.n,
                                         float(rho), int(adaptive), L.ptr(self.scratch),
                                         L.ptr(self.out3), stream())

    def restore(self):
        L = _L()
        return L.lib().cilrs_sam_restore(L.ptr(self.p), L.ptr(self.backup), self.n, stream())

    def check(self):
        for c in (self.check_p, self.check_g, self.check_b, self.check_s, self.check_o):
            c()
        self.const.check()
        tail = self.scratch[self.nchunks * 8:]
        assert bool((tail == PATTERN).all()), "scratch written behind the chunk sums"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. norm, scale and the perturbed parameters ---------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n", SIZES)
def test_perturb_is_the_definition(n, rho, adaptive):
    p, g = make_data(n)
    want64, s_exact, _, _ = reference(n, rho, adaptive)
    c = Call(p, g)
    assert c.perturb(rho, adaptive) == 0
    c.check()
    assert torch.equal(bits(c.backup), bits(p)), "backup is not the pre-call p"
    s_dev, norm, scale = c.out3.cpu().tolist()
    print(f"n={n} rho={rho} adaptive={adaptive}: S {s_dev!r} (fsum {s_exact!r}), norm {norm!r}, "
          f"scale {scale!r}")
    assert abs(s_dev - s_exact) <= 2.0 ** -40 * s_exact
    assert abs(norm - math.sqrt(s_dev)) <= math.ulp(math.sqrt(s_dev))
    assert scale == rho / (norm + 1e-12)
    got = c.p.cpu()
    want32 = S.perturb32(p, g, S.s32_of(scale), adaptive)
    assert torch.equal(bits(got), bits(want32)), \
        f"{int((bits(got) != bits(want32)).sum())} elements differ from the fp32 statement"
    Q.gate("p", got, want64, S.perturb32(p, g, S.s32_of(reference(n, rho, adaptive)[3]), adaptive))
    if rho == 0.0:
        assert torch.equal(got, p)


# ---- 2. identities and the restore -----------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("rho", [0.05, 2.0])
def test_zero_gradient_leaves_p_unchanged_and_finite(rho, adaptive):
    n = CHUNK + 4
    p, _ = make_data(n)
    c = Call(p, torch.zeros(n))
    assert c.perturb(rho, adaptive) == 0
    c.check()
    assert c.out3.cpu().tolist() == [0.0, 0.0, rho / 1e-12]
    got = c.p.cpu()
    assert torch.equal(got, p) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("adaptive", [0, 1])
def test_restore_gives_back_every_bit(adaptive):
    n = 3 * CHUNK + 12
    p, g = make_data(n)
    p = p.clone()
    special = torch.tensor([-0x80000000, 0x00000001, 0x007FFFFF, -0x7FFFFFFF, 0x7FC12345, 0x7FA00001,
                            -0x00400001, 0x7F800000, -0x00800000, 0x00000000], dtype=torch.int32)
    special = special.view(torch.float32)        # -0.0, denormals, quiet / signalling NaNs, +-inf, 0
    for at in (0, 2051, CHUNK - 3, CHUNK + 1, n - len(special)):
        p[at:at + len(special)] = special
    c = Call(p, g)
    assert c.perturb(0.05, adaptive) == 0
    assert torch.equal(bits(c.backup), bits(p)), "backup lost bits"
    assert not torch.equal(bits(c.p), bits(p))
    assert c.restore() == 0
    c.check()
    assert torch.equal(bits(c.p), bits(p)), "restore lost bits"


# ---- 3. guards: one call per case ------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_nothing_outside_the_buffers_is_written(n, adaptive):
    p, g = make_data(n)
    c = Call(p, g)
    assert c.perturb(0.05, adaptive) == 0
    c.check()
    assert bool(torch.isfinite(c.backup).all()) and bool(torch.isfinite(c.out3).all())
    assert c.restore() == 0
    c.check()
    assert torch.equal(bits(c.p), bits(p))


# ---- 4. determinism and range independence ---------------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
def test_two_runs_and_a_sub_range_are_bit_identical(adaptive):
    n, b = 3 * CHUNK + 12, 2052                   # the sub-range starts mid-chunk of the larger arena
    p, g = make_data(n)
    runs = []
    for _ in range(2):
        c = Call(p, g)
        assert c.perturb(0.05, adaptive) == 0
        c.check()
        runs.append((bits(c.p), bits(c.backup), c.out3.cpu().view(torch.int64)))
    for x, y in zip(*runs):
        assert torch.equal(x, y), "two runs differ"
    # the same data as [b, b + n) of a larger arena, through offset pointers
    L = _L()
    big_p, big_g = make_data(b + n, seed=7)
    big_p, big_g = big_p.clone(), big_g.clone()
    big_p[b:], big_g[b:] = p, g
    P, check_p = gbuf(big_p, "arena params")
    G, check_g = gbuf(big_g, "arena grads")
    B, check_b = guarded(b + n, fill=float("nan"), guard=4096, name="arena backup")
    scratch, check_s = guarded(L.lib().cilrs_sam_scratch_bytes(n), dtype=torch.uint8, fill=None,
                               name="scratch")
    out3, check_o = guarded(3, dtype=torch.float64, fill=float("nan"), name="out3")
    assert L.lib().cilrs_sam_perturb(L.ptr(P[b:]), L.ptr(G[b:]), L.ptr(B[b:]), n, 0.05, adaptive,
                                     L.ptr(scratch), L.ptr(out3), stream()) == 0
    for chk in (check_p, check_g, check_b, check_s, check_o):
        chk()
    assert torch.equal(bits(P[:b]), bits(big_p[:b])), "params in front of the range were written"
    assert bool(torch.isnan(B[:b]).all()), "backup in front of the range was written"
    assert torch.equal(bits(P[b:]), runs[0][0]) and torch.equal(bits(B[b:]), runs[0][1])
    assert torch.equal(out3.cpu().view(torch.int64), runs[0][2])


# ---- 5. refusals: non-zero, a message that names the argument, nothing launched -------------------------
def _refused(rc, needle):
    assert rc != 0
    msg = (_L().lib().cilrs_last_error() or b"").decode()
    assert needle in msg, msg


def test_refusals_happen_before_any_launch():
    L = _L()
    lib = L.lib()
    n = CHUNK + 4
    p_cpu, g_cpu = make_data(n)
    c = Call(p_cpu, g_cpu)
    c.backup.copy_(torch.arange(n, dtype=torch.float32))
    before = (bits(c.p), bits(c.backup), c.out3.cpu().view(torch.int64).clone())
    P, G, B, SCR, O3 = (L.ptr(t) for t in (c.p, c.g, c.backup, c.scratch, c.out3))

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def call(params=P, grads=G, backup=B, count=n, rho=0.05, adaptive=0, scratch=SCR, out3=O3):
        return lib.cilrs_sam_perturb(params, grads, backup, count, rho, adaptive, scratch, out3,
                                     stream())

    for kw in (dict(params=None), dict(grads=None), dict(backup=None), dict(scratch=None),
               dict(out3=None)):
        _refused(call(**kw), "NULL")
    _refused(call(count=0), "multiple of 4")
    _refused(call(count=n - 2), "multiple of 4")
    _refused(call(count=2 ** 30 + 4), "2^30")
    _refused(call(params=off(c.p, 4), count=n - 4), "aligned")
    _refused(call(grads=off(c.g, 8), count=n - 4), "aligned")
    _refused(call(backup=off(c.backup, 12), count=n - 4), "aligned")
    _refused(call(scratch=off(c.scratch, 8)), "scratch")
    _refused(call(out3=off(c.out3, 4)), "out3")
    _refused(call(backup=P), "overlaps")
    _refused(call(backup=off(c.p, 16), count=n - 4), "overlaps")
    _refused(call(params=off(c.p, 4096), backup=P, count=n - 1024), "overlaps")
    _refused(call(backup=G), "overlaps")
    _refused(call(backup=off(c.g, 4 * (n - 4)), count=8, grads=off(c.g, 4 * (n - 8))), "overlaps")
    for rho in (-0.05, -1e-300, float("nan"), float("inf"), float("-inf")):
        _refused(call(rho=rho), "rho")
    for adaptive in (2, -1, 256):
        _refused(call(adaptive=adaptive), "adaptive")

    def restore(params=P, backup=B, count=n):
        return lib.cilrs_sam_restore(params, backup, count, stream())

    _refused(restore(params=None), "NULL")
    _refused(restore(backup=None), "NULL")
    _refused(restore(count=0), "multiple of 4")
    _refused(restore(count=6), "multiple of 4")
    _refused(restore(params=off(c.p, 4), count=n - 4), "aligned")
    _refused(restore(backup=off(c.backup, 4), count=n - 4), "aligned")
    _refused(restore(backup=P), "overlaps")
    _refused(restore(backup=off(c.p, 16), count=n - 4), "overlaps")
    c.check()
    assert torch.equal(bits(c.p), before[0]), "params were written by a refused call"
    assert torch.equal(bits(c.backup), before[1]), "backup was written by a refused call"
    assert torch.equal(c.out3.cpu().view(torch.int64), before[2]), "out3 was written"
    assert bool((c.scratch == PATTERN).all()), "scratch was written by a refused call"


# ====================================================================================================
# Trainer level: B = 8 synthetic batches, portable weights
# ====================================================================================================
@pytest.fixture(scope="module")
def weights():
    from cilrs_mi355 import CILRS
    return O.portable_state_dict(CILRS(4, 0.0).state_dict(), 0)


def make_model(weights, dropout=0.0):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=dropout)
    m.load_state_dict(weights, strict=True)
    return m.cuda()


@functools.lru_cache(maxsize=None)
def batches(k, seed0=70):
    return [[t.cuda() for t in O.synthetic_batch(8, seed=seed0 + i)[:4]] for i in range(k)]


def cfg_with(base, **kw):
    from cilrs_mi355 import TrainConfig
    return TrainConfig(**{**base.__dict__, **kw})


def snapshot(tr):
    return dict(params=tr.eng.params.cpu(), exp_avg=tr.exp_avg.cpu(), exp_avg_sq=tr.exp_avg_sq.cpu())


def bn_state(eng):
    return dict(bn=eng.bn.cpu(), nbt=eng.nbt.cpu())


class Pieces:
    """The two entry points on a model's arena, with buffers of the test's own."""

    def __init__(self, eng):
        L = _L()
        self.eng = eng
        self.backup = torch.full((eng.n_arena,), float("nan"), device=eng.device)
        nbytes = L.lib().cilrs_sam_scratch_bytes(eng.n_arena)
        self.scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=eng.device)
        self.out3 = torch.zeros(3, dtype=torch.float64, device=eng.device)

    def perturb(self, rho, adaptive, e=0, g=0):
        L, eng = _L(), self.eng
        b = eng.trainable_begin(g)
        L.check(L.lib().cilrs_sam_perturb(L.ptr(eng.params[b:]), L.ptr(eng.grads[b:]),
                                          L.ptr(self.backup[b:]), eng.n_arena - b, float(rho),
                                          int(adaptive), L.ptr(self.scratch), L.ptr(self.out3),
                                          stream()))
        eng.wrote_trainable(e)

    def restore(self, e=0, g=0):
        L, eng = _L(), self.eng
        b = eng.trainable_begin(g)
        L.check(L.lib().cilrs_sam_restore(L.ptr(eng.params[b:]), L.ptr(self.backup[b:]),
                                          eng.n_arena - b, stream()))
        eng.wrote_trainable(e)


def composed_sam_step(tr, pieces, batch, rho, adaptive):
    """One SAM step from public pieces on a PLAIN Trainer: forward, loss, backward; perturb; forward
    with the same seed (BatchNorm buffers saved and put back around it), loss, backward; restore;
    optimizer_step.  -> (loss at w, loss at w + e, g2)"""
    imgs, spds, cmds, tgts = batch
    eng, cfg = tr.eng, tr.cfg
    assert cfg.sam_rho == 0.0
    if not tr.model.training:                     # (train() on a frozen model would thaw its prefix)
        tr.model.train()
    e, g = tr.model.freeze_state()
    seed = tr.next_dropout_seed() if cfg.dropout > 0 else 0
    c, s, pl = eng.run_forward_ft(imgs, spds, cmds, e, g, cfg.dropout, seed)
    buf, dc, dp = tr.loss(c, tgts, s, spds)
    loss1 = buf.clone()
    eng.run_backward(pl, dc, dp)
    pieces.perturb(rho, adaptive, e, g)
    # the second forward must not count as a batch: an eval-mode prefix of a LATER step reads the
    # running statistics.  Put back through torch here (the Trainer's own route is another one).
    bn, nbt = eng.bn.clone(), eng.nbt.clone()
    c, s, pl = eng.run_forward_ft(imgs, spds, cmds, e, g, cfg.dropout, seed)
    eng.bn.copy_(bn)
    eng.nbt.copy_(nbt)
    buf, dc, dp = tr.loss(c, tgts, s, spds)
    loss2 = buf.clone()
    eng.run_backward(pl, dc, dp)
    g2 = eng.grads.clone()
    pieces.restore(e, g)
    tr.optimizer_step()
    return loss1, loss2, g2


def assert_same_state(a, b, what):
    sa, sb = snapshot(a), snapshot(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs"


# ---- 6. one SAM step is the composition ------------------------------------------------------------
ONE_STEP = {
    "adam": (dict(), {}, None),
    "adaptive-clip": (dict(sam_adaptive=True, grad_clip=1.0), {}, None),
    "lamb": (dict(optimizer="lamb"), {}, None),
    "dropout": (dict(dropout=0.5), {}, None),
    "bf16": (dict(), dict(precision="bf16"), None),
    "frozen-layer1": (dict(optimizer="lamb"), {}, "layer1"),
}


@pytest.mark.parametrize("case", list(ONE_STEP))
def test_one_sam_step_is_the_composition(weights, case):
    from cilrs_mi355 import CILRS, CONFIG_A, Trainer
    kw, tkw, freeze = ONE_STEP[case]
    rho = 0.05
    plain = cfg_with(CONFIG_A, **kw)
    adaptive = plain.sam_adaptive
    drop = plain.dropout
    data = batches(2)
    ma, mb = make_model(weights, drop), make_model(weights, drop)
    ta = Trainer(ma, cfg_with(plain, sam_rho=rho), **tkw)
    tb = Trainer(mb, cfg_with(plain, sam_adaptive=False), **tkw)
    pieces = Pieces(tb.eng)
    frozen = 0
    if freeze is not None:                            # one SAM step with everything trainable first
        ta.train_step(*data[0])
        composed_sam_step(tb, pieces, data[0], rho, adaptive)
        assert_same_state(ta, tb, "the step before the freeze")
        for m in (ma, mb):
            m.train()
            m.freeze(freeze)
        frozen = 2                                    # stem and layer1
    # a third model: the same weights and buffers, ONE plain step on the batch
    mc = CILRS(num_commands=4, dropout=drop)
    mc.load_state_dict({k: v.detach().cpu().contiguous() for k, v in ma.state_dict().items()})
    mc = mc.cuda()
    if freeze is not None:
        mc.train()
        mc.freeze(freeze)
    tc = Trainer(mc, cfg_with(plain, sam_adaptive=False), **tkw)
    assert torch.equal(tc.eng.params, ta.eng.params) and torch.equal(tc.eng.bn, ta.eng.bn)
    before, nbt0, seeds0, steps0 = snapshot(ta), ta.eng.nbt.cpu(), ta._seed_calls, ta.sam_steps
    batch = data[1]
    out = ta.train_step(*batch)
    loss1, loss2, g2 = composed_sam_step(tb, pieces, batch, rho, adaptive)
    tc.train_step(*batch)
    torch.cuda.synchronize()
    assert out is ta.loss_buf and ta.sam_steps == steps0 + 1 and ta.step_count == tb.step_count
    assert torch.equal(ta.eng.grads, g2), "the gradient arena is not the gradient at w + e"
    assert torch.equal(ta.loss_buf[:6], loss1[:6]), "loss_buf is not the loss at w"
    assert torch.equal(ta.sam_loss_buf[:6], loss2[:6]), "sam_loss_buf is not the loss at w + e"
    assert not torch.equal(loss1[:6], loss2[:6]), "the second pass did not see the perturbed weights"
    assert_same_state(ta, tb, case)
    assert torch.equal(ta.sam_norm(), pieces.out3.cpu())
    # BatchNorm buffers: as ONE plain forward at w leaves them
    assert torch.equal(ta.eng.bn, tc.eng.bn), "running statistics differ from one plain step's"
    assert torch.equal(ta.eng.nbt, tc.eng.nbt)
    assert torch.equal(tb.eng.bn, tc.eng.bn) and torch.equal(tb.eng.nbt, tc.eng.nbt)
    trained = (ta.eng.nbt.cpu() - nbt0)
    assert set(trained.tolist()) <= {0, 1} and int(trained.max()) == 1, "not exactly one more batch"
    if freeze is None:
        assert bool((trained == 1).all())
    # one seed serves both passes
    assert ta._seed_calls == seeds0 + (1 if drop > 0 else 0) and ta._seed_calls == tc._seed_calls
    if freeze is not None:
        begin = ta.eng.trainable_begin(frozen)
        after = snapshot(ta)
        assert begin > 0 and ta.group_steps == [1, 1, 2, 2, 2, 2]
        for k in after:
            assert torch.equal(after[k][:begin], before[k][:begin]), f"frozen range of {k} moved"
        assert bool((trained[:1] == 0).all()), "the frozen stem's BatchNorm counted a batch"
    assert not torch.equal(snapshot(ta)["params"], before["params"])


# ---- 7. off is the parent's step -------------------------------------------------------------------
def test_sam_off_is_the_parents_step(weights):
    from cilrs_mi355 import CONFIG_A, TrainConfig, Trainer
    spelled = cfg_with(CONFIG_A, sam_rho=0.0, sam_adaptive=False, sam_every=1)
    assert spelled == TrainConfig()
    out = []
    for cfg in (CONFIG_A, spelled):
        tr = Trainer(make_model(weights), cfg)
        for b in batches(2):
            tr.train_step(*b)
        assert tr.sam_backup is None and tr._sam_scratch is None and tr.sam_steps == 0
        with pytest.raises(RuntimeError, match="no SAM perturbation"):
            tr.sam_norm()
        out.append(snapshot(tr))
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


# ---- 8. sam_every ----------------------------------------------------------------------------------
def test_sam_every_two_over_three_steps(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    data = batches(3)
    ta = Trainer(make_model(weights), cfg_with(CONFIG_A, sam_rho=0.05, sam_every=2))
    tb = Trainer(make_model(weights), CONFIG_A)
    pieces = Pieces(tb.eng)
    want_sam = [1, 1, 2]
    for t, b in enumerate(data):
        ta.train_step(*b)
        if t % 2 == 0:
            composed_sam_step(tb, pieces, b, 0.05, False)
        else:
            tb.train_step(*b)
        assert ta.sam_steps == want_sam[t]
        assert_same_state(ta, tb, f"step {t + 1}")
    assert ta.step_count == 3 and ta.sam_steps == 2


# ---- 9. EMA and the fuse_optimizer refusal ------------------------------------------------------------
def test_ema_rides_on_the_sam_step_and_fuse_optimizer_is_refused(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    tr = Trainer(make_model(weights), cfg_with(CONFIG_A, sam_rho=0.05, ema_decay=0.9,
                                               ema_warmup=True))
    ema = tr.eng.params.cpu()
    data = batches(2)
    for t, b in enumerate(data, 1):
        tr.train_step(*b)
        ema = E.step32(ema, tr.eng.params.cpu(), E.weight32(0.9, t, True))
        assert tr.ema_updates == t and tr.sam_steps == t
        assert torch.equal(tr.ema.cpu(), ema), f"update {t}"
    assert not torch.equal(tr.ema, tr.eng.params)
    with pytest.raises(RuntimeError, match="ema_weights"):
        with tr.ema_weights():
            tr.train_step(*data[0])
    for t in (tr, Trainer(make_model(weights), cfg_with(CONFIG_A, sam_rho=0.05))):
        state = (snapshot(t), t.eng.grads.clone(), t.eng.bn.clone(), t.loss_buf.clone())
        counts = (t.step_count, t.sam_steps, t._seed_calls, t.eng.weights_epoch)
        t.fuse_optimizer = True
        with pytest.raises(RuntimeError, match="fuse_optimizer cannot serve sam_rho"):
            t.train_step(*data[0])
        with pytest.raises(RuntimeError, match="fuse_optimizer cannot serve sam_rho"):
            t.optimizer_step()
        t.fuse_optimizer = False
        torch.cuda.synchronize()
        now = snapshot(t)
        assert all(torch.equal(now[k], state[0][k]) for k in now)
        assert torch.equal(t.eng.grads, state[1]) and torch.equal(t.eng.bn, state[2])
        assert torch.equal(t.loss_buf, state[3])
        assert counts == (t.step_count, t.sam_steps, t._seed_calls, t.eng.weights_epoch)


# ---- 10. data parallel, world size 1 ---------------------------------------------------------------
def test_data_parallel_routes_equal_the_single_gpu_route(weights, tmp_path):
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer
    cfg = cfg_with(CONFIG_A, sam_rho=0.05)
    data = batches(2)
    out = {}
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for bucket in (True, False):
            tr = Trainer(make_model(weights), cfg, process_group=dist.group.WORLD)
            tr.bucket_optimizer = bucket
            collectives = []
            for b in data:
                tr.train_step(*b)
                collectives.append(tr.reducer.collectives)
            torch.cuda.synchronize()
            assert tr.step_count == 2 and tr.sam_steps == 2
            # the first pass is this rank's own: only the second one's three buckets are reduced
            assert collectives == [3, 6]
            out[bucket] = (snapshot(tr), bn_state(tr.eng), tr.sam_norm())
    finally:
        dist.destroy_process_group()
    single = Trainer(make_model(weights), cfg)
    for b in data:
        single.train_step(*b)
    out["single"] = (snapshot(single), bn_state(single.eng), single.sam_norm())
    for route in (False, "single"):
        for k in out[True][0]:
            assert torch.equal(out[True][0][k], out[route][0][k]), f"{k}: bucket route != {route}"
        for k in out[True][1]:
            assert torch.equal(out[True][1][k], out[route][1][k]), f"{k}: bucket route != {route}"
        assert torch.equal(out[True][2], out[route][2])


# ---- 11. Trainer.sharpness -------------------------------------------------------------------------
def everything(tr):
    d = snapshot(tr)
    d.update(bn_state(tr.eng))
    if tr.ema is not None:
        d["ema"] = tr.ema.cpu()
    return d, (tr.step_count, tr.sam_steps, tr.ema_updates, tuple(tr.group_lag), tr._seed_calls)


def test_sharpness_is_the_composition_and_leaves_the_state_alone(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    data = batches(2)
    tr = Trainer(make_model(weights), cfg_with(CONFIG_A, ema_decay=0.9))
    tr.train_step(*data[0])                           # moments and an average that differ from zero / p
    twin = Trainer(make_model({k: v.detach().cpu().contiguous()
                               for k, v in tr.model.state_dict().items()}), CONFIG_A)
    assert torch.equal(twin.eng.params, tr.eng.params) and torch.equal(twin.eng.bn, tr.eng.bn)
    before = everything(tr)
    assert tr.sam_backup is None                      # SAM is off in this config
    zero = tr.sharpness(data, rho=0.0)
    assert zero["sharpness"] == 0.0 and zero["loss"] == zero["loss_perturbed"] and zero["batches"] == 2
    res = tr.sharpness(data, rho=0.05, adaptive=False)
    # the composition on the twin, accumulated the same way
    pieces = Pieces(twin.eng)
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    for imgs, spds, cmds, tgts in data:
        c, s, pl = twin.eng.run_forward_frozen(imgs, spds, cmds)
        buf, dc, dp = twin.loss(c, tgts, s, spds)
        acc[0:1] += buf[0:1].double()
        twin.eng.run_backward(pl, dc, dp)
        pieces.perturb(0.05, False)
        c, s, pl = twin.eng.run_forward_frozen(imgs, spds, cmds)
        buf, _, _ = twin.loss(c, tgts, s, spds, want_grads=False)
        acc[1:2] += buf[0:1].double()
        acc[2:3] += pieces.out3[1:2]
        pieces.restore()
    a, b, c = (acc / 2).tolist()
    assert (res["loss"], res["loss_perturbed"], res["grad_norm"]) == (a, b, c)
    assert res["sharpness"] == b - a and res["batches"] == 2
    assert res["loss"] == zero["loss"] and res["sharpness"] > 0.0 and res["grad_norm"] > 0.0
    assert torch.equal(tr.sam_norm(), pieces.out3.cpu())
    after = everything(tr)
    assert after[1] == before[1]
    for k in before[0]:
        assert torch.equal(after[0][k], before[0][k]), f"sharpness changed {k}"
    # inside ema_weights(): the averaged weights' sharpness; both arenas as they were
    with tr.ema_weights():
        inside = everything(tr)
        avg = tr.sharpness(data[:1], rho=0.05, adaptive=True)
        again = everything(tr)
        for k in inside[0]:
            assert torch.equal(again[0][k], inside[0][k]), f"sharpness inside ema_weights changed {k}"
    assert avg["batches"] == 1 and math.isfinite(avg["sharpness"]) and avg["loss"] != res["loss"]
    after = everything(tr)
    for k in before[0]:
        assert torch.equal(after[0][k], before[0][k]), f"{k} after ema_weights()"
    with pytest.raises(ValueError, match="sam_rho"):
        tr.sharpness(data, rho=-1.0)
    with pytest.raises(ValueError, match="no batches"):
        tr.sharpness([])


def test_sharpness_over_the_trainable_range_of_a_frozen_prefix(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    m = make_model(weights)
    tr = Trainer(m, CONFIG_A)
    m.train()
    m.freeze("layer1")
    begin = tr.eng.trainable_begin(2)
    before = everything(tr)
    res = tr.sharpness(batches(1), rho=0.05)
    # the backup beyond the cut is the weights; in front of it nothing was ever written
    assert torch.equal(tr.sam_backup[begin:], tr.eng.params[begin:])
    full = Trainer(make_model(weights), CONFIG_A).sharpness(batches(1), rho=0.05)
    # fewer coordinates share the same radius: another perturbation, from the same loss at w
    assert res["loss"] == full["loss"] and res["grad_norm"] < full["grad_norm"]
    assert res["sharpness"] != full["sharpness"]
    after = everything(tr)
    for k in before[0]:
        assert torch.equal(after[0][k], before[0][k]), f"sharpness changed {k}"


def test_both_losses_of_a_perturbation_against_the_float64_oracle(weights):
    """L(w) and L(w + e) of the device against cilrs_oracle in float64 on the CPU, eval mode, at the
    tolerance tests/test_model_gpu.py holds the loss to at this batch size (B = 8, step 1: lines
    179-181, 1e-4 * max(1, |loss|))."""
    from cilrs_mi355 import CONFIG_A, Trainer
    m = make_model(weights)
    tr = Trainer(m, CONFIG_A)
    imgs, spds, cmds, tgts = batches(1)[0]
    pieces = Pieces(tr.eng)
    c, s, pl = tr.eng.run_forward_frozen(imgs, spds, cmds)
    buf, dc, dp = tr.loss(c, tgts, s, spds)
    got_w = dict(zip(("total", "control", "steer", "throttle", "brake", "speed"), buf[:6].tolist()))
    tr.eng.run_backward(pl, dc, dp)
    pieces.perturb(0.05, False)
    perturbed = {k: v.detach().cpu().contiguous().double() for k, v in m.state_dict().items()}
    c, s, pl = tr.eng.run_forward_frozen(imgs, spds, cmds)
    buf, _, _ = tr.loss(c, tgts, s, spds, want_grads=False)
    got_e = dict(zip(got_w, buf[:6].tolist()))
    pieces.restore()
    orc = O.build_oracle(0).double().eval()
    cpu = [t.cpu() for t in (imgs, spds, cmds, tgts)]

    def oracle_loss():
        with torch.no_grad():
            pc, ps = orc(cpu[0].double(), cpu[1].double(), cpu[2])
            return O.compute_loss(O.CONFIG_A, pc, cpu[3].double(), ps, cpu[1].double())[1]

    want_w = oracle_loss()
    orc.load_state_dict(perturbed, strict=True)
    want_e = oracle_loss()
    print(f"L(w): device {got_w['total']!r} oracle {want_w['total']!r}; "
          f"L(w + e): device {got_e['total']!r} oracle {want_e['total']!r}")
    assert want_e["total"] > want_w["total"]
    for got, want in ((got_w, want_w), (got_e, want_e)):
        for k, v in want.items():
            assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
