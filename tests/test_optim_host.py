"""AdamW / LAMB / warm-up / cosine, host side: the schedules against closed forms, TrainConfig
validation before anything is built, the segment flags of the ResNet-34 layout, the checkpoint
config keys, the chunk count of the table-size query, and the two CPU statements of tests/_optim.py
against torch.optim.AdamW and against each other."""
import ctypes as C
import math
import types

import pytest
import torch

import _optim as Q


def _stub(cfg, step_count=0, epoch=0):
    """A Trainer without a device: what lr_now / scheduler_step touch"""
    from cilrs_mi355 import Trainer
    tr = Trainer.__new__(Trainer)
    tr.cfg, tr.lr, tr.step_count, tr.epoch = cfg, cfg.lr, step_count, epoch
    return tr


def test_warmup_and_cosine_against_a_closed_form_table():
    from cilrs_mi355 import TrainConfig
    cfg = TrainConfig(optimizer="lamb", lr=8e-3, warmup_steps=4, lr_schedule="cosine", lr_epochs=4,
                      lr_min=8e-4)
    tr = _stub(cfg)
    assert tr.lr == 8e-3 and tr.lr_now == 8e-3 * 0.25          # before the first step: step 1's
    want_steps = {1: 2e-3, 2: 4e-3, 3: 6e-3, 4: 8e-3, 5: 8e-3, 100: 8e-3}
    for t, want in want_steps.items():
        tr.step_count = t
        assert tr.lr_now == pytest.approx(want, rel=1e-15) and tr.lr_at(t) == tr.lr_now
    assert tr.lr_at(4) == tr.lr and tr.lr_at(9) == tr.lr       # the warm-up over: lr itself, exactly
    # cosine: lr_min + (lr - lr_min) * {1, (2+sqrt2)/4, 1/2, (2-sqrt2)/4, 0}
    frac = [1.0, (2 + math.sqrt(2)) / 4, 0.5, (2 - math.sqrt(2)) / 4, 0.0, 0.0, 0.0]
    tr.step_count = 2                                            # still warming up: lr_now = lr / 2
    for epoch in range(1, 7):
        tr.scheduler_step()
        want = 8e-4 + (8e-3 - 8e-4) * frac[epoch]
        assert tr.epoch == epoch and tr.lr == pytest.approx(want, rel=1e-12, abs=1e-18)
        assert tr.lr_now == pytest.approx(0.5 * want, rel=1e-12, abs=1e-18)


def test_cosine_at_and_beyond_lr_epochs_is_lr_min_and_steplr_is_unchanged():
    from cilrs_mi355 import CONFIG_A, TrainConfig
    from cilrs_mi355.train import cosine_lr, scheduled_lr, steplr
    cfg = TrainConfig(lr=1e-3, lr_schedule="cosine", lr_epochs=7, lr_min=1e-5)
    assert cosine_lr(cfg, 0) == 1e-3
    for e in (7, 8, 100):
        assert cosine_lr(cfg, e) == 1e-5 == scheduled_lr(cfg, e)
    assert all(cosine_lr(cfg, e) > cosine_lr(cfg, e + 1) for e in range(7))
    # the default schedule is StepLR(8, 0.5), value for value
    for e in range(0, 30):
        assert scheduled_lr(CONFIG_A, e) == steplr(CONFIG_A, e) == 2e-4 * 0.5 ** (e // 8)
    tr = _stub(CONFIG_A, step_count=3)
    assert tr.lr_now == CONFIG_A.lr                             # no warm-up: the scheduled rate
    for e in range(1, 10):
        tr.scheduler_step()
        assert tr.lr == steplr(CONFIG_A, e) == tr.lr_now


@pytest.mark.parametrize("kw,needle", [
    (dict(optimizer="sgd"), "optimizer"),
    (dict(optimizer="LAMB"), "optimizer"),
    (dict(lr_schedule="linear"), "lr_schedule"),
    (dict(warmup_steps=-1), "warmup_steps"),
    (dict(warmup_steps=2.5), "warmup_steps"),
    (dict(optimizer="lamb", trust_clip=-1.0), "trust_clip"),
    (dict(optimizer="lamb", trust_clip=float("nan")), "trust_clip"),
    (dict(decay_exempt_1d=True), "decay_exempt_1d"),
    (dict(optimizer="adam", decay_exempt_1d=True), "decay_exempt_1d"),
    (dict(lr_schedule="cosine", lr_epochs=0), "lr_epochs"),
    (dict(lr_schedule="cosine", lr_min=1.0), "lr_min"),
])
def test_bad_options_are_refused_before_anything_is_built(kw, needle):
    from cilrs_mi355 import TrainConfig, Trainer

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} touched before the options were validated")

    with pytest.raises(ValueError, match=needle):
        Trainer(Untouchable(), TrainConfig(**kw))


def test_defaults_are_todays_behaviour():
    from cilrs_mi355 import CONFIG_A, CONFIG_B, TrainConfig
    for cfg in (CONFIG_A, CONFIG_B, TrainConfig()):
        assert cfg.optimizer == "adam" and cfg.decay_exempt_1d is False and cfg.trust_clip == 0.0
        assert cfg.warmup_steps == 0 and cfg.lr_schedule == "step"


def test_segment_flags_of_the_resnet34_layout_mark_exactly_the_1d_tensors():
    from cilrs_mi355 import CILRS
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.engine import _layout
    from cilrs_mi355.train import SEG_NO_ADAPT, SEG_NO_DECAY, segment_table
    layout = _layout()[0]
    n = L.lib().cilrs_param_arena_floats()
    shapes = [tuple(p.shape) for p in CILRS().parameters()]
    assert len(layout) == len(shapes) == 142
    ends, flags = segment_table(layout, n, True, lamb=True)
    assert len(ends) == len(flags) == 142 and ends[-1] == n
    assert all(e % 4 == 0 for e in ends) and all(a < b for a, b in zip(ends, ends[1:]))
    for (name, off, numel, _), end in zip(layout, ends):
        assert off + numel <= end < off + numel + 4, name      # a tensor, then < 4 padding floats
    one_d = [len(s) <= 1 for s in shapes]
    assert one_d == [len(p[3]) <= 1 for p in layout]
    # 36 BatchNorm layers (weight and bias) and the heads' Linear biases; no convolution, no matrix
    n_linear = sum(len(s) == 2 for s in shapes)
    assert sum(one_d) == 2 * 36 + n_linear and sum(len(s) == 4 for s in shapes) == 36
    assert flags == [(SEG_NO_DECAY | SEG_NO_ADAPT) if d else 0 for d in one_d]
    assert segment_table(layout, n, True, lamb=False)[1] == [SEG_NO_DECAY if d else 0 for d in one_d]
    assert segment_table(layout, n, False, lamb=True)[1] == [0] * 142
    # the table-size query counts one 16-byte entry per segment and per chunk of a segment
    chunk = L.lib().cilrs_optim_chunk_floats()
    starts = [0] + ends[:-1]
    chunks = sum(-(-(e - b) // chunk) for b, e in zip(starts, ends))
    c_ends = (C.c_size_t * 142)(*ends)
    assert L.lib().cilrs_optim_table_bytes(c_ends, 142) == 16 * (142 + chunks)
    bad = (C.c_size_t * 3)(8, 8, 16)
    assert L.lib().cilrs_optim_table_bytes(bad, 3) == 0 and L.lib().cilrs_optim_table_bytes(None, 3) == 0


CONFIG_KEYS = {"name", "lr", "weight_decay", "loss", "loss_weights", "grad_clip", "dropout", "betas",
               "eps", "lr_step_size", "lr_gamma", "lr_mult"}


def test_config_dict_keeps_its_key_set_at_defaults_and_records_only_what_is_set():
    from cilrs_mi355 import CONFIG_A, CONFIG_B, TrainConfig
    from cilrs_mi355.checkpoint import _config_dict
    for cfg in (CONFIG_A, CONFIG_B):
        assert set(_config_dict(types.SimpleNamespace(cfg=cfg))) == CONFIG_KEYS
    cfg = TrainConfig(optimizer="lamb", warmup_steps=3, lr_schedule="cosine")
    d = _config_dict(types.SimpleNamespace(cfg=cfg))
    assert set(d) == CONFIG_KEYS | {"optimizer", "warmup_steps", "lr_schedule"}
    assert d["optimizer"] == "lamb" and d["warmup_steps"] == 3 and d["lr_schedule"] == "cosine"
    cfg = TrainConfig(optimizer="adamw", decay_exempt_1d=True, trust_clip=0.0, lr_min=0.0)
    assert set(_config_dict(types.SimpleNamespace(cfg=cfg))) == CONFIG_KEYS | {"optimizer",
                                                                                "decay_exempt_1d"}


def test_resuming_under_another_optimizer_is_a_value_error():
    from cilrs_mi355 import TrainConfig
    from cilrs_mi355.checkpoint import _check_same_optimizer
    lamb = types.SimpleNamespace(cfg=TrainConfig(optimizer="lamb"))
    adam = types.SimpleNamespace(cfg=TrainConfig())
    _check_same_optimizer(lamb, {"config": {"optimizer": "lamb"}}, "f.pth")
    _check_same_optimizer(adam, {}, "f.pth")                    # no key: counts as "adam"
    _check_same_optimizer(adam, {"config": {"lr": 1.0}}, "f.pth")
    with pytest.raises(ValueError, match="optimizer='lamb'"):
        _check_same_optimizer(adam, {"config": {"optimizer": "lamb"}}, "f.pth")
    with pytest.raises(ValueError, match="optimizer='adam'"):
        _check_same_optimizer(lamb, {}, "f.pth")


def _case(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = 0.05 * torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 1, (n,), generator=g).float()
    gr[::7] = 0.0
    return p, gr


def test_the_cpu_statements_agree_with_torch_adamw_and_with_each_other():
    """tests/_optim.py is the oracle of the device tests; here it is checked itself, with the flag
    constants of the package: AdamW fp32 and float64 against torch.optim.AdamW over five steps
    (1e-6, the project's gate for cilrs_adam_step), LAMB fp32 against float64."""
    from cilrs_mi355.train import OPTIM_KIND, SEG_NO_ADAPT, SEG_NO_DECAY
    assert (Q.NO_DECAY, Q.NO_ADAPT) == (SEG_NO_DECAY, SEG_NO_ADAPT)
    assert OPTIM_KIND == {"adamw": Q.ADAMW, "lamb": Q.LAMB}
    hp = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-6, wd=1e-2)
    n = 4100
    for flags in (0, Q.NO_DECAY):
        p0, _ = _case(n, 3)
        ref = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([ref], lr=hp["lr"], betas=(0.9, 0.999), eps=hp["eps"],
                                weight_decay=0.0 if flags else hp["wd"], foreach=False)
        p32, m32, v32 = p0.clone(), torch.zeros(n), torch.zeros(n)
        p64, m64, v64 = p0.double(), torch.zeros(n).double(), torch.zeros(n).double()
        for t in range(1, 6):
            _, g = _case(n, 10 + t)
            ref.grad = g * 0.25
            opt.step()
            p32, m32, v32, _ = Q.step32(Q.ADAMW, p32, g, m32, v32, step=t, gs=0.25, flags=flags, **hp)
            p64, m64, v64, _ = Q.step64(Q.ADAMW, p64, g, m64, v64, step=t, gs=0.25, flags=flags, **hp)
            st = opt.state[ref]
            for a, b in ((p32, ref.detach()), (m32, st["exp_avg"]), (v32, st["exp_avg_sq"])):
                assert float((a - b).abs().max()) <= 1e-6
            assert float((p64 - ref.detach().double()).abs().max()) <= 1e-6
    # LAMB: the ratio of the fp32 statement within 1e-6 relative of float64, p within 8 * 2^-24 max|p|
    for flags, clip in ((0, 0.0), (Q.NO_DECAY, 0.0), (0, 0.5), (Q.NO_DECAY | Q.NO_ADAPT, 0.0)):
        p, _ = _case(n, 4)
        m, v = torch.zeros(n), torch.zeros(n)
        for t in range(1, 6):
            _, g = _case(n, 20 + t)
            a = Q.step32(Q.LAMB, p, g, m, v, step=t, flags=flags, trust_clip=clip, **hp)
            b = Q.step64(Q.LAMB, p, g, m, v, step=t, flags=flags, trust_clip=clip, **hp)
            assert abs(a[3] - b[3]) <= 1e-6 * b[3]
            assert (a[3] == 1.0) == bool(flags & Q.NO_ADAPT)
            assert float((a[0].double() - b[0]).abs().max()) <= 8 * 2.0 ** -24 * float(b[0].abs().max())
            p, m, v = a[0], a[1], a[2]
    # degenerate norms: p == 0, and u == 0 (no gradient, no decay) -> ratio exactly 1, p untouched
    z = torch.zeros(n)
    assert Q.step32(Q.LAMB, z, g, z, z, step=1, **hp)[3] == 1.0
    out = Q.step32(Q.LAMB, p, z, z, z, step=1, flags=Q.NO_DECAY, **hp)
    assert out[3] == 1.0 and torch.equal(out[0], p)
