"""EMA of the weights, host side: the oracle of tests/_ema.py against itself (fp32 chain inside the
derived bound of the float64 chain), the warmup schedule, TrainConfig.ema_decay validation, and
the ema_state_dict key / shape contract on a Trainer without a device."""
import math
import types

import pytest
import torch

import _ema as E


def _mixed(n, seed):
    """N(0,1) scaled by magnitudes 1e-6 .. 1e3, with exact zeros"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 4, (n,), generator=g).float()
    x[::17] = 0.0
    return x


@pytest.mark.parametrize("d,warmup", [(0.5, False), (0.9, False), (0.999, False)])
def test_fp32_chain_stays_inside_the_derived_bound_of_the_float64_chain(d, warmup):
    """w <= 0.5 in every case, as the derivation of _ema.bound needs"""
    n, T = 4096, 8
    ema0 = _mixed(n, 1)
    ps = [_mixed(n, 10 + t) for t in range(T)]
    ps[0][5::17] = ema0[5::17]                  # ema == p elements
    ws = [E.weight32(d, t + 1, warmup) for t in range(T)]
    assert all(w <= 0.5 for w in ws)
    e32, e64 = E.chain32(ema0, ps, ws), E.chain64(ema0, ps, ws)
    Ms = E.running_max(ema0, ps, e32)
    assert torch.equal(e32[0][5::17], ema0[5::17]), "ema == p must come back bit-identical"
    worst = max(E.worst_ratio(e32[t], e64[t], t + 1, Ms[t]) for t in range(T))
    print(f"d={d}: worst |fp32 - float64| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_warmup_schedule_first_values_and_the_package_agrees():
    from cilrs_mi355.train import ema_decay_at, ema_weight
    assert E.decay_at(0.999, 1) == 2.0 / 11.0
    assert E.decay_at(0.999, 2) == 3.0 / 12.0
    assert E.decay_at(0.999, 8) == 0.5
    assert E.decay_at(0.1, 1) == 0.1                       # the cap is the configured decay
    assert E.decay_at(0.999, 10 ** 6) == 0.999
    assert E.decay_at(0.999, 1, warmup=False) == 0.999
    for d in (0.0, 0.1, 0.9, 0.999, 0.9999):
        for warm in (True, False):
            for t in (1, 2, 3, 9, 10, 100, 8990, 8991, 10 ** 5):
                assert ema_decay_at(d, t, warm) == E.decay_at(d, t, warm)
                w = ema_weight(d, t, warm)
                assert w == E.weight32(d, t, warm)
                assert float(torch.tensor(w, dtype=torch.float32)) == w     # an fp32 value
                assert abs(w - (1.0 - E.decay_at(d, t, warm))) <= 2.0 ** -24
    assert ema_weight(0.999, 1) == float(torch.tensor(9.0 / 11.0, dtype=torch.float32))


@pytest.mark.parametrize("bad", [1.0, 1.5, -0.1, float("nan"), float("inf"), -float("inf"), "x"])
def test_bad_ema_decay_is_refused_before_anything_is_built(bad):
    from cilrs_mi355 import TrainConfig, Trainer

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} touched before ema_decay was validated")

    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(Untouchable(), TrainConfig(ema_decay=bad))


def test_ema_config_defaults_and_accepted_values():
    from cilrs_mi355 import CONFIG_A, CONFIG_B, TrainConfig
    from cilrs_mi355.train import check_ema_decay
    assert CONFIG_A.ema_decay is None and CONFIG_B.ema_decay is None
    assert TrainConfig().ema_warmup is True
    for ok in (0, 0.0, 0.5, 0.999, 1.0 - 2.0 ** -30):
        assert check_ema_decay(ok) == float(ok) and math.isfinite(check_ema_decay(ok))


def _stub_trainer(seed):
    """A Trainer around a CPU arena: what ema_state_dict / load_ema_state_dict touch, no device"""
    from cilrs_mi355 import Trainer
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.engine import _layout
    n = L.lib().cilrs_param_arena_floats()
    tr = Trainer.__new__(Trainer)
    tr.eng = types.SimpleNamespace(params_layout=_layout()[0], n_arena=n, params=None)
    tr.ema = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    tr.ema_updates, tr._in_ema = 0, False
    return tr


def test_ema_state_dict_keys_shapes_and_round_trip_on_a_cpu_stub():
    from cilrs_mi355 import CILRS
    m = CILRS()
    a, b = _stub_trainer(1), _stub_trainer(2)
    sd = a.ema_state_dict()
    named = list(m.named_parameters())
    assert list(sd) == [n for n, _ in named] and len(sd) == 142
    for n, p in named:
        assert tuple(sd[n].shape) == tuple(p.shape) and sd[n].dtype == torch.float32
        assert sd[n].is_contiguous()
    assert not any(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in sd)
    m.load_state_dict(sd, strict=False)                      # keyed and shaped like the model's own
    b.load_ema_state_dict(sd)
    back = b.ema_state_dict()
    assert all(torch.equal(sd[k], back[k]) for k in sd)
    with pytest.raises(KeyError):
        b.load_ema_state_dict({k: v for k, v in list(sd.items())[1:]})
    with pytest.raises(KeyError):
        b.load_ema_state_dict({**sd, "visual_encoder.1.running_mean": torch.zeros(64)})
    wrong = dict(sd)
    wrong[named[0][0]] = torch.zeros(3)
    with pytest.raises(ValueError):
        b.load_ema_state_dict(wrong)
    from cilrs_mi355 import Trainer
    off = Trainer.__new__(Trainer)
    off.ema = None
    with pytest.raises(RuntimeError, match="no EMA"):
        off.ema_state_dict()


def test_ema_weights_unlocks_the_trainer_even_when_the_swap_back_fails():
    from cilrs_mi355 import Trainer
    tr = Trainer.__new__(Trainer)
    tr.ema, tr._in_ema = torch.zeros(4), False
    tr._ensure_engine = lambda: None
    calls = []

    def swap():
        calls.append(len(calls))
        if len(calls) == 2:
            raise RuntimeError("device error in the exchange back")
    tr._swap_ema = swap
    with pytest.raises(RuntimeError, match="exchange back"):
        with tr.ema_weights():
            assert tr._in_ema
    assert calls == [0, 1] and tr._in_ema is False
