"""EMA of the weights on the device: the four C-ABI entries (cilrs_ema_update, cilrs_adam_step_ema,
cilrs_adam_step_groups_ema, cilrs_swap) against the fp32 definition of tests/_ema.py and against the
unfused entries, inside guard bands; then the Trainer: every optimizer route, through the separate
pass (the default) and through the fused launches (Trainer.ema_fused), ema_weights(), checkpoints,
fit and resume.

Everything that can be bit-exact is compared with torch.equal: the definition is three separately
rounded fp32 operations, which the CPU restates exactly.  The one tolerance is the derived bound of
_ema.bound against the float64 chain (cases with w <= 0.5, as its derivation needs).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _ema as E
import cilrs_oracle as O
from _guards import Inputs, guarded

pytestmark = pytest.mark.gpu

# the smallest vector, a ragged single block, and the smallest size that enters the grid-stride
# loop of a 4096-block launch (4096 * 256 threads of 4 floats, then 257 more quads)
SIZES = [4, 1020, 4 * 4096 * 256 + 1028]
LR, B1, B2, EPS, WD = 2e-4, 0.9, 0.999, 1e-8, 1e-4


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _mixed(n, seed):
    """CPU fp32: N(0,1) scaled by magnitudes 1e-6 .. 1e3, with exact zeros"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 4, (n,), generator=g).float()
    x[::17] = 0.0
    return x


def _gbuf(cpu, name):
    v, check = guarded(cpu.numel(), fill=None, guard=4096, name=name)
    v.copy_(cpu)
    return v, check


# ---- cilrs_ema_update ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_is_the_fp32_definition_bit_for_bit(n):
    L = _L()
    T = 3
    ema0 = _mixed(n, 1)
    ps = [_mixed(n, 10 + t) for t in range(T)]
    ps[0][1::5] = ema0[1::5]                                   # ema == p: must come back untouched
    ws = [E.weight32(0.999, t + 1, True) for t in range(T)]    # 9/11, 9/12, 9/13
    want = E.chain32(ema0, ps, ws)
    ema, check = _gbuf(ema0, "ema")
    for t in range(T):
        p = ps[t].cuda()
        const = Inputs(params=p)
        L.check(L.lib().cilrs_ema_update(L.ptr(ema), L.ptr(p), n, ws[t], stream()))
        check()
        const.check()
        got = ema.cpu()
        assert torch.equal(got, want[t]), f"step {t + 1}: {int((got != want[t]).sum())} of {n} differ"
        if t == 0:
            assert torch.equal(got[1::5].view(torch.int32), ema0[1::5].view(torch.int32))


# ---- cilrs_adam_step_ema / cilrs_adam_step_groups_ema ---------------------------------------------
def _adam(L, fused, table, p, g, m, v, n, step, clip, gscale, ema=None, w=0.0):
    lib = L.lib()
    args = [L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n]
    if table is None:
        fn = lib.cilrs_adam_step_ema if fused else lib.cilrs_adam_step
        args += [LR, B1, B2, EPS, WD, step]
    else:
        fn = lib.cilrs_adam_step_groups_ema if fused else lib.cilrs_adam_step_groups
        k = len(table)
        args += [k, (C.c_size_t * k)(*table), (C.c_double * k)(*[LR * (i + 1) for i in range(k)]),
                 (C.c_int64 * k)(*[step + i for i in range(k)]), B1, B2, EPS, WD]
    args += [L.ptr(clip), gscale]
    if fused:
        args += [L.ptr(ema), w]
    return fn(*args, stream())


ADAM_SHAPES = [(n, None) for n in SIZES] + [
    (5004, (2500, 5004)),                                                       # 2 ranges
    (70004, (1004, 5012, 9020, 20004, 33332, 40100, 66668, 70004)),             # 8 ranges
    (SIZES[2], (2000004, SIZES[2])),                          # a range end inside the second trip's data
]


@pytest.mark.parametrize("clip_on,gscale", [(False, 1.0), (False, 0.5), (True, 1.0), (True, 0.5)])
@pytest.mark.parametrize("n,table", ADAM_SHAPES, ids=lambda x: None if x is None else (
    str(x) if isinstance(x, int) else f"{len(x)}ranges"))
def test_adam_step_ema_equals_adam_then_ema_update_and_the_float64_bound(n, table, clip_on, gscale):
    L = _L()
    if table is not None:
        assert all(e % 4 == 0 and e % 1024 != 0 for e in table) and table[-1] == n
    T = 3
    ws = [E.weight32(d, 1, False) for d in (0.5, 0.9, 0.99)]           # all <= 0.5: _ema.bound
    p0, ema0 = _mixed(n, 2), _mixed(n, 3)
    ema0[1::5] = p0[1::5]
    m0 = torch.randn(n, generator=torch.Generator().manual_seed(4)) * 1e-2
    v0 = torch.rand(n, generator=torch.Generator().manual_seed(5)) * 1e-3
    clip = torch.tensor([2.0, 0.5], device="cuda") if clip_on else None
    # unfused: the existing entries on plain tensors
    pu, mu, vu, eu = p0.cuda(), m0.cuda(), v0.cuda(), ema0.cuda()
    # fused: inside guard bands
    (pf, cp), (mf, cm), (vf, cv), (ef, ce) = (_gbuf(p0, "params"), _gbuf(m0, "exp_avg"),
                                              _gbuf(v0, "exp_avg_sq"), _gbuf(ema0, "ema"))
    ps = []
    for t in range(T):
        g = torch.randn(n, generator=torch.Generator().manual_seed(20 + t)).cuda()
        const = Inputs(grads=g, clip_out2=clip)
        L.check(_adam(L, False, table, pu, g, mu, vu, n, 3 + t, clip, gscale))
        L.check(L.lib().cilrs_ema_update(L.ptr(eu), L.ptr(pu), n, ws[t], stream()))
        L.check(_adam(L, True, table, pf, g, mf, vf, n, 3 + t, clip, gscale, ef, ws[t]))
        for c in (cp, cm, cv, ce):
            c()
        const.check()
        assert torch.equal(pf, pu) and torch.equal(mf, mu) and torch.equal(vf, vu), \
            f"step {t + 1}: the fused launch moved the Adam trajectory"
        assert torch.equal(ef, eu), f"step {t + 1}: fused ema != cilrs_ema_update after the step"
        ps.append(pf.cpu())
    assert not torch.equal(ps[-1], p0)
    # the device's own parameter sequence through the CPU definitions
    e32, e64 = E.chain32(ema0, ps, ws), E.chain64(ema0, ps, ws)
    assert torch.equal(ef.cpu(), e32[-1])
    Ms = E.running_max(ema0, ps, e32)
    worst = max(E.worst_ratio(e32[t], e64[t], t + 1, Ms[t]) for t in range(T))
    print(f"n={n} ranges={0 if table is None else len(table)} clip={clip_on} gscale={gscale}: "
          f"worst |ema - float64| / (4 T 2^-24 M) = {worst:.4f}")
    assert worst <= 1.0


# ---- cilrs_swap ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_exactly_and_twice_is_the_identity(n):
    L = _L()
    a0, b0 = _mixed(n, 6), _mixed(n, 7)
    a0[0], b0[-1] = float("nan"), float("inf")                 # bits travel, values are not looked at
    (a, ca), (b, cb) = _gbuf(a0, "a"), _gbuf(b0, "b")
    L.check(L.lib().cilrs_swap(L.ptr(a), L.ptr(b), n, stream()))
    ca(), cb()
    assert torch.equal(a.cpu().view(torch.int32), b0.view(torch.int32))
    assert torch.equal(b.cpu().view(torch.int32), a0.view(torch.int32))
    L.check(L.lib().cilrs_swap(L.ptr(a), L.ptr(b), n, stream()))
    ca(), cb()
    assert torch.equal(a.cpu().view(torch.int32), a0.view(torch.int32))
    assert torch.equal(b.cpu().view(torch.int32), b0.view(torch.int32))


# ---- refusals: non-zero, a message, nothing launched -----------------------------------------------
def _refused(L, rc, needle):
    assert rc != 0
    msg = (L.lib().cilrs_last_error() or b"").decode()
    assert needle in msg, msg


def test_refusals_launch_nothing():
    L = _L()
    lib = L.lib()
    n = 1024
    cpu = {k: _mixed(n + 8, 30 + i) for i, k in enumerate(("p", "m", "v", "e", "g"))}
    cpu["v"] = cpu["v"].abs()
    bufs = {k: _gbuf(t, k) for k, t in cpu.items()}
    p, m, v, e, g = (bufs[k][0] for k in ("p", "m", "v", "e", "g"))

    def untouched():
        for k, (t, check) in bufs.items():
            check()
            assert torch.equal(t.cpu().view(torch.int32), cpu[k].view(torch.int32)), f"{k} was written"

    # cilrs_ema_update
    _refused(L, lib.cilrs_ema_update(L.ptr(e), L.ptr(p), 1022, 0.1, stream()), "multiple of 4")
    _refused(L, lib.cilrs_ema_update(None, L.ptr(p), n, 0.1, stream()), "NULL")
    _refused(L, lib.cilrs_ema_update(L.ptr(p), L.ptr(p), n, 0.1, stream()), "alias")
    _refused(L, lib.cilrs_ema_update(L.ptr(p[4:]), L.ptr(p), n, 0.1, stream()), "alias")
    _refused(L, lib.cilrs_ema_update(L.ptr(e), L.ptr(p), n, 1.5, stream()), "outside")
    _refused(L, lib.cilrs_ema_update(L.ptr(e), L.ptr(p), n, float("nan"), stream()), "outside")
    untouched()
    # the fused Adam entries: single range, then a 2-range table
    for table in (None, (500, 1024)):
        odd = None if table is None else (500, 1022)
        _refused(L, _adam(L, True, odd, p, g, m, v, 1022, 3, None, 1.0, e, 0.1), "multiple of 4")
        _refused(L, _adam(L, True, table, p, g, m, v, n, 3, None, 1.0, None, 0.1), "NULL")
        for alias in (p, m, v, m[4:], p[4:]):
            _refused(L, _adam(L, True, table, p, g, m, v, n, 3, None, 1.0, alias, 0.1), "alias")
        untouched()
    # cilrs_swap
    _refused(L, lib.cilrs_swap(L.ptr(p), L.ptr(e), 1022, stream()), "multiple of 4")
    _refused(L, lib.cilrs_swap(L.ptr(p), None, n, stream()), "NULL")
    _refused(L, lib.cilrs_swap(None, L.ptr(e), n, stream()), "NULL")
    _refused(L, lib.cilrs_swap(L.ptr(p), L.ptr(p), n, stream()), "overlap")
    _refused(L, lib.cilrs_swap(L.ptr(p), L.ptr(p[4:]), n, stream()), "overlap")
    untouched()


# ====================================================================================================
# Trainer level: B = 4 synthetic batches, portable weights
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


def batches(k, seed0=70):
    return [[t.cuda() for t in O.synthetic_batch(4, seed=seed0 + i)[:4]] for i in range(k)]


def cfg_with(base, **kw):
    from cilrs_mi355 import TrainConfig
    return TrainConfig(**{**base.__dict__, **kw})


def training_state(tr):
    eng = tr.eng
    return dict(params=eng.params.clone(), grads=eng.grads.clone(), exp_avg=tr.exp_avg.clone(),
                exp_avg_sq=tr.exp_avg_sq.clone(), bn=eng.bn.clone(), nbt=eng.nbt.clone(),
                loss_buf=tr.loss_buf.clone())


def same_training_state(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: `{k}` differs between EMA on and EMA off"


class Replay:
    """the fp32 definition replayed on the CPU from per-step parameter snapshots"""

    def __init__(self, tr, d, warmup):
        self.tr, self.d, self.warmup = tr, d, warmup
        self.ema = tr.eng.params.cpu()
        self.t = 0

    def step_and_compare(self, what=""):
        self.t += 1
        self.ema = E.step32(self.ema, self.tr.eng.params.cpu(), E.weight32(self.d, self.t, self.warmup))
        got = self.tr.ema.cpu()
        assert self.tr.ema_updates == self.t
        assert torch.equal(got, self.ema), \
            f"{what} update {self.t}: {int((got != self.ema).sum())} elements differ from the definition"


FUSED = pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])


@FUSED
@pytest.mark.parametrize("cfg_name", ["A", "B"])
def test_ema_does_not_move_the_training_trajectory(weights, cfg_name, fused):
    """Config A, and B as executed (clipping, dropout 0.5): three steps with the EMA on and three
    with it off leave parameters, moments, gradients, BatchNorm buffers and losses identical."""
    from cilrs_mi355 import CONFIG_A, CONFIG_B, Trainer
    base = CONFIG_A if cfg_name == "A" else CONFIG_B
    data = batches(3)
    states = {}
    for on in (False, True):
        torch.manual_seed(123)
        m = make_model(weights, dropout=base.dropout)
        tr = Trainer(m, cfg_with(base, ema_decay=0.99) if on else base)
        assert (tr.ema is not None) == on and tr.ema_fused is False      # the measured default
        tr.ema_fused = fused
        rep = Replay(tr, 0.99, True) if on else None
        states[on] = []
        for b in data:
            tr.train_step(*b)
            states[on].append(training_state(tr))
            if on:
                rep.step_and_compare(f"config {cfg_name}")
    for t in range(3):
        same_training_state(states[False][t], states[True][t], f"config {cfg_name} step {t + 1}")


@FUSED
@pytest.mark.parametrize("d,warmup", [(0.999, True), (0.9, False), (0.0, False)])
def test_trainer_ema_is_the_definition_after_every_step(weights, d, warmup, fused):
    """The test that fails without the feature."""
    from cilrs_mi355 import CONFIG_A, Trainer
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=d, ema_warmup=warmup))
    tr.ema_fused = fused
    assert tr.ema.dtype == torch.float32 and tr.ema.numel() == tr.eng.n_arena
    assert tr.ema.data_ptr() != tr.eng.params.data_ptr() and torch.equal(tr.ema, tr.eng.params)
    rep = Replay(tr, d, warmup)
    for b in batches(3):
        tr.train_step(*b)
        rep.step_and_compare()
    if d > 0.0:
        assert not torch.equal(tr.ema, tr.eng.params)
    tr.ema_reset()
    assert tr.ema_updates == 0 and torch.equal(tr.ema, tr.eng.params)


@FUSED
def test_table_route_frozen_prefix_and_the_step_after(weights, fused):
    """lr_mult takes the table-driven launch; freeze("layer2") the ranged Adam plus the pass over
    the frozen prefix; unfreezing gives the groups different step counts (table again)."""
    from cilrs_mi355 import CONFIG_A, Trainer
    data = batches(5)
    mult = {"stem": 0.1, "layer1": 0.1}
    out = {}
    for on in (False, True):
        m = make_model(weights)
        tr = Trainer(m, cfg_with(CONFIG_A, lr_mult=mult, ema_decay=0.9 if on else None,
                                 ema_warmup=False))
        tr.ema_fused = fused
        rep = Replay(tr, 0.9, False) if on else None
        out[on] = []
        for i, b in enumerate(data):
            if i == 2:
                m.train()
                m.freeze("layer2")
            if i == 4:
                m.unfreeze()
            before = tr.ema.clone() if on else None
            tr.train_step(*b)
            out[on].append(training_state(tr))
            if on:
                rep.step_and_compare(f"step {i + 1}")
                if i in (2, 3):
                    begin = tr.eng.trainable_begin(3)
                    assert begin > 0 and tr.group_lag[:3] == [i - 1] * 3
                    assert torch.equal(tr.eng.params[:begin], out[on][1]["params"][:begin])
                    moved = (tr.ema[:begin] != before[:begin]).float().mean()
                    assert float(moved) > 0.5, "the frozen prefix's average did not move"
    for t in range(5):
        same_training_state(out[False][t], out[True][t], f"step {t + 1}")


@FUSED
@pytest.mark.parametrize("bucket_optimizer", [True, False])
def test_data_parallel_bucket_route_world1(weights, tmp_path, bucket_optimizer, fused):
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer
    cfg = cfg_with(CONFIG_A, ema_decay=0.9, ema_warmup=True)
    data = batches(3)
    m1 = make_model(weights)
    single = Trainer(m1, cfg)
    for b in data:
        single.train_step(*b)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        m2 = make_model(weights)
        tr = Trainer(m2, cfg, process_group=dist.group.WORLD)
        tr.bucket_optimizer = bucket_optimizer
        tr.ema_fused = fused
        rep = Replay(tr, 0.9, True)
        for b in data:
            tr.train_step(*b)
            rep.step_and_compare("data parallel")
        torch.cuda.synchronize()
        assert tr.ema_updates == tr.step_count == 3
        assert torch.equal(tr.eng.params, single.eng.params)
        assert torch.equal(tr.ema, single.ema)
    finally:
        dist.destroy_process_group()


def test_fuse_optimizer_with_ema_raises_before_any_launch(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=0.9))
    tr.fuse_optimizer = True
    before = training_state(tr)
    with pytest.raises(RuntimeError, match="fuse_optimizer"):
        tr.train_step(*batches(1)[0])
    torch.cuda.synchronize()
    same_training_state(before, training_state(tr), "refused step")
    assert tr.step_count == 0 and tr.ema_updates == 0 and torch.equal(tr.ema, tr.eng.params)


@FUSED
def test_bf16_precision_keeps_an_fp32_ema(weights, fused):
    from cilrs_mi355 import CONFIG_A, Trainer
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=0.9, ema_warmup=False), precision="bf16")
    tr.ema_fused = fused
    rep = Replay(tr, 0.9, False)
    tr.train_step(*batches(1)[0])
    assert tr.ema.dtype == torch.float32
    rep.step_and_compare("bf16")


def _averaged_twin(weights, tr, m):
    """a fresh model: the averaged parameters + the live model's BatchNorm buffers"""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ema_sd = tr.ema_state_dict()
    assert set(ema_sd) == {n for n, _ in m.named_parameters()}
    sd.update(ema_sd)
    return make_model(sd).eval()


def test_ema_weights_context(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    from cilrs_mi355.predict import Predictor
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=0.9, ema_warmup=False))
    data = batches(3)
    for b in data:
        tr.train_step(*b)
    twin = _averaged_twin(weights, tr, m)
    imgs, spds, cmds, _ = batches(1, seed0=90)[0]
    u8 = O.synthetic_batch(1, seed=1)[4]
    m.eval()
    pred = Predictor(m)                                        # batch 1: the persistent launch
    raw_tick = pred.predict_batch(u8, [30.0], [2]).copy()
    with torch.no_grad():
        raw_out = [t.clone() for t in m(imgs, spds, cmds)]
        want = [t.clone() for t in twin(imgs, spds, cmds)]
    want_tick = Predictor(twin).predict_batch(u8, [30.0], [2]).copy()
    assert not np.array_equal(raw_tick, want_tick) and not torch.equal(raw_out[0], want[0])
    arena, ema = tr.eng.params.clone(), tr.ema.clone()
    epoch = tr.eng.weights_epoch
    with tr.ema_weights():
        assert tr.eng.weights_epoch > epoch
        assert torch.equal(tr.eng.params, ema) and torch.equal(tr.ema, arena)
        with torch.no_grad():
            got = m(imgs, spds, cmds)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert np.array_equal(pred.predict_batch(u8, [30.0], [2]), want_tick)
        sd_in = tr.ema_state_dict()                            # still the averaged parameters
        assert all(torch.equal(sd_in[k], v.cpu()) for k, v in twin.state_dict().items()
                   if k in sd_in)
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step(*data[0])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.optimizer_step()
        with pytest.raises(RuntimeError, match="re-entrant"):
            with tr.ema_weights():
                pass
        assert torch.equal(tr.eng.params, ema), "a refused call disturbed the swapped arena"
    assert torch.equal(tr.eng.params, arena) and torch.equal(tr.ema, ema)
    assert np.array_equal(pred.predict_batch(u8, [30.0], [2]), raw_tick)
    with torch.no_grad():
        back = m(imgs, spds, cmds)
    assert torch.equal(back[0], raw_out[0]) and torch.equal(back[1], raw_out[1])
    # an exception inside still restores the arena
    with pytest.raises(KeyError, match="boom"):
        with tr.ema_weights():
            raise KeyError("boom")
    assert torch.equal(tr.eng.params, arena) and torch.equal(tr.ema, ema)
    # validate(ema=True) is validate() of the averaged model
    val = batches(2, seed0=20)
    got_v, _ = tr.validate(val, ema=True)
    assert torch.equal(tr.eng.params, arena)
    want_v, _ = Trainer(twin, CONFIG_A).validate(val)
    raw_v, _ = tr.validate(val)
    assert got_v == want_v and got_v != raw_v
    tr.train_step(*data[0])                                    # training goes on afterwards


# ---- fit, checkpoints, resume ----------------------------------------------------------------------
BEST_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "val_steer", "config",
             "cmd_steer_errors"}
LATEST_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict",
               "loop_state"}
CONFIG_KEYS = {"name", "lr", "weight_decay", "loss", "loss_weights", "grad_clip", "dropout", "betas",
               "eps", "lr_step_size", "lr_gamma", "lr_mult"}


def _fit(weights, out_dir, epochs, ema=True, resume=None):
    from cilrs_mi355 import CONFIG_A, Trainer
    from cilrs_mi355.loop import fit
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=0.9) if ema else CONFIG_A)
    train, val = batches(2, seed0=70), batches(2, seed0=20)
    seen = {}

    def log(line):
        if line.startswith("epoch ") and ema:      # after validate, before the checkpoints
            ep = int(line.split()[1].split("/")[0])
            seen[ep] = (tr.ema_state_dict(),
                        {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                        tr.ema_updates)
    res = fit(tr, lambda: train, lambda: val, epochs=epochs, patience=6, out_dir=str(out_dir),
              resume=resume, log=log)
    return m, tr, res, seen


def test_fit_checkpoints_and_resume_continue_the_ema_trajectory(weights, tmp_path):
    from cilrs_mi355 import CILRS
    from cilrs_mi355.checkpoint import load_file
    m, tr, res, seen = _fit(weights, tmp_path / "a", 2)
    best = load_file(tmp_path / "a" / "checkpoint_best.pth")
    latest = load_file(tmp_path / "a" / "checkpoint_latest.pth")
    # best: the averaged parameters of its epoch under the model's 250 keys, live BatchNorm buffers
    ep = best["epoch"]
    assert ep == res["best_epoch"] and set(best) == BEST_KEYS | {"ema"}
    ema_sd, model_sd, updates = seen[ep]
    assert best["ema"] == {"decay": 0.9, "updates": updates} and updates == 2 * ep
    fresh = CILRS(4, 0.0)
    fresh.load_state_dict(best["model_state_dict"], strict=True)
    assert list(best["model_state_dict"]) == list(model_sd) and len(model_sd) == 250
    for k, v in best["model_state_dict"].items():
        assert torch.equal(v, ema_sd[k] if k in ema_sd else model_sd[k]), k
    assert any(not torch.equal(best["model_state_dict"][k], model_sd[k]) for k in ema_sd)
    assert best["config"]["ema_decay"] == 0.9 and best["config"]["ema_warmup"] is True
    # latest: the raw weights, the average beside them
    assert set(latest) == LATEST_KEYS | {"ema_state_dict", "ema_updates"}
    assert latest["ema_updates"] == 4 == tr.ema_updates
    now = tr.ema_state_dict()
    assert list(latest["ema_state_dict"]) == list(now)
    assert all(torch.equal(latest["ema_state_dict"][k], now[k]) for k in now)
    assert all(torch.equal(v, m.state_dict()[k].cpu()) for k, v in latest["model_state_dict"].items())
    # resume for one more epoch == three epochs without interruption, bit for bit
    _, tr_resumed, _, _ = _fit(weights, tmp_path / "b", 3,
                               resume=str(tmp_path / "a" / "checkpoint_latest.pth"))
    _, tr_whole, _, _ = _fit(weights, tmp_path / "c", 3)
    assert tr_resumed.ema_updates == tr_whole.ema_updates == 6
    assert torch.equal(tr_resumed.eng.params, tr_whole.eng.params)
    assert torch.equal(tr_resumed.ema, tr_whole.ema)


def test_without_ema_the_files_have_todays_keys_and_loading_one_resets_the_average(weights, tmp_path):
    from cilrs_mi355 import CONFIG_A, Trainer, checkpoint
    from cilrs_mi355.checkpoint import load_file
    _, tr, _, _ = _fit(weights, tmp_path, 1, ema=False)
    assert tr.ema is None and tr.ema_updates == 0
    best = load_file(tmp_path / "checkpoint_best.pth")
    latest = load_file(tmp_path / "checkpoint_latest.pth")
    assert set(best) == BEST_KEYS and set(latest) == LATEST_KEYS
    assert set(best["config"]) == CONFIG_KEYS
    assert len(best["model_state_dict"]) == 250 == len(latest["model_state_dict"])
    # a trainer with an EMA that loads a file without one starts the average from the loaded weights
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, ema_decay=0.9))
    tr.train_step(*batches(1)[0])
    assert tr.ema_updates == 1 and not torch.equal(tr.ema, tr.eng.params)
    checkpoint.load(str(tmp_path / "checkpoint_latest.pth"), m, tr)
    assert tr.ema_updates == 0 and torch.equal(tr.ema, tr.eng.params)
