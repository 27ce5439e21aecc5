"""FGSM / PGD, host side: the fp32 and float64 statements of tests/_adversarial.py against each
other and on the identities of the definition, cilrs_adv_direction's cases, the TrainConfig
defaults and refusals before anything is built, the adv_every schedule, the default step sizes of
Predictor.adversarial and the refusals of the C ABI that need no device."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import _adversarial as A

U = 2.0 ** -24          # one fp32 rounding, relative


def _data(B, H, W, seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[0, 0, 0] = (0, 255, 0)                    # the ends of the range are in every batch
    frames[-1, -1, -1] = (255, 0, 255)
    x = A.preprocess(frames)
    g = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    return frames, x, g


@pytest.mark.parametrize("eps255,alpha255", [(0.5, 0.5), (2.0, 0.5), (8.0, 3.0), (300.0, 40.0)])
@pytest.mark.parametrize("clamp", [False, True])
def test_the_fp32_statement_is_within_fp32_rounding_of_the_float64_one(eps255, alpha255, clamp):
    _, x, g = _data(2, 7, 9, 3)
    rng = A.RANGE6 if clamp else None
    x64 = x.astype(np.float64)
    s32, s64 = A.start_ref(x, eps255, 11, rng), A.start_ref(x64, eps255, 11, rng, np.float64)
    e = A.per_channel(eps255, np.float64)
    a = A.per_channel(alpha255, np.float64)
    # e_c carries two roundings (the scale, the product); e * r, the sum and each bound one more:
    # at most 4 roundings of magnitudes below |x| + e
    bound = 4 * U * (np.abs(x64) + e) + 1e-45
    err = np.abs(s32.astype(np.float64) - s64)
    assert (err <= bound).all(), float((err / bound).max())
    row_dir = np.array([1.0, -1.0], dtype=np.float32)
    t32, _ = A.step_ref(x, s32, g, alpha255, eps255, row_dir, None, None, rng)
    t64, _ = A.step_ref(x64, s32.astype(np.float64), g, alpha255, eps255, row_dir, None, None, rng,
                        np.float64)
    bound = 4 * U * (np.abs(x64) + e + a) + 1e-45
    err = np.abs(t32.astype(np.float64) - t64)
    assert (err <= bound).all(), float((err / bound).max())
    assert not np.array_equal(t32, s32)
    # the deviation: 4 differences, 4 products, 3 sums -- each one rounding of at most sum |w (c - r)|
    r = np.random.default_rng(5)
    c, rc = r.standard_normal((6, 3)).astype(np.float32), r.standard_normal((6, 3)).astype(np.float32)
    s, rs = r.standard_normal(6).astype(np.float32), r.standard_normal(6).astype(np.float32)
    w = (0.5, -1.0, 0.25, 2.0)
    d32 = A.direction_ref(c, s, rc, rs, w, True, None)[0]
    d64 = A.direction_ref(c, s, rc, rs, w, True, None, np.float64)[0]
    mag = np.abs(np.asarray(w[:3]) * (c.astype(np.float64) - rc)).sum(1) + abs(w[3]) * np.abs(
        s.astype(np.float64) - rs)
    assert (np.abs(d32 - d64) <= 11 * U * mag).all()


@pytest.mark.parametrize("eps255", [0.0, 0.5, 2.0, 300.0])
@pytest.mark.parametrize("clamp", [False, True])
def test_every_iterate_stays_in_the_eps_ball(eps255, clamp):
    _, x, g = _data(2, 5, 8, 7)
    rng = A.RANGE6 if clamp else None
    e = A.per_channel(eps255)
    xa = A.start_ref(x, eps255, 99, rng)
    if eps255 == 0:
        assert xa.tobytes() == x.tobytes()           # a copy, bit for bit
    for k in range(4):
        assert (xa >= x - e).all() and (xa <= x + e).all()       # fp32 comparison, fp32 bounds
        if clamp:
            lo = np.asarray(A.RANGE6[0::2], dtype=np.float32).reshape(1, 3, 1, 1)
            hi = np.asarray(A.RANGE6[1::2], dtype=np.float32).reshape(1, 3, 1, 1)
            assert (xa >= lo).all() and (xa <= hi).all()
        xa, _ = A.step_ref(x, xa, np.roll(g, k), 1.5 * eps255 + 0.25, eps255, None, None, None, rng)
    assert (xa >= x - e).all() and (xa <= x + e).all()


def test_alpha_zero_zero_and_nan_gradients_leave_the_iterate():
    _, x, g = _data(2, 4, 6, 2)
    xa = A.start_ref(x, 2.0, 5)
    best = np.full_like(xa, 7.0)
    out, b2 = A.step_ref(x, xa, g, 0.0, 2.0, None, np.array([1, 0], dtype=np.int32), best)
    assert out.tobytes() == xa.tobytes()
    assert np.array_equal(b2[0], xa[0]) and (b2[1] == 7.0).all()     # the copy still happens
    out, _ = A.step_ref(x, xa, None, 0.0, 2.0)                       # g may be absent then
    assert out.tobytes() == xa.tobytes()
    for fill in (0.0, -0.0, float("nan")):
        out, _ = A.step_ref(x, xa, np.full_like(g, fill), 1.0, 2.0)
        assert np.array_equal(out, xa)
    # infinities are signs like any other
    out, _ = A.step_ref(x, xa, np.full_like(g, float("inf")), 0.25, 300.0)
    assert (out > xa).all()
    out, _ = A.step_ref(x, xa, np.full_like(g, float("-inf")), 0.25, 300.0)
    assert (out < xa).all()


@pytest.mark.parametrize("eps", [1, 2, 8])
def test_quantised_bytes_move_at_most_eps_levels(eps):
    frames, x, g = _data(2, 6, 10, 13)
    assert (frames == 0).any() and (frames == 255).any()
    q, linf = A.quantize_ref(x, frames)
    assert np.array_equal(q, frames) and (linf == 0).all()           # the preprocessing inverts
    xa = A.start_ref(x, float(eps), 3, A.RANGE6)
    for k in range(3):
        xa, _ = A.step_ref(x, xa, np.roll(g, 5 * k), float(eps), float(eps), None, None, None, A.RANGE6)
        q, linf = A.quantize_ref(xa, frames)
        diff = np.abs(q.astype(np.int32) - frames.astype(np.int32))
        assert diff.max() <= eps
        assert np.array_equal(linf, diff.reshape(2, -1).max(1))
    assert linf.max() == eps                         # a full step reaches the ball's surface
    # the float64 statement rounds to the same bytes except at exact ties
    q64, _ = A.quantize_ref(xa.astype(np.float64), frames, np.float64)
    assert np.abs(q64.astype(np.int32) - q.astype(np.int32)).max() <= 1
    # NaN and out-of-range inputs: 0, and the clip
    bad = np.array([float("nan"), -1e9, 1e9], dtype=np.float32).reshape(1, 3, 1, 1)
    assert A.quantize_ref(bad)[0].reshape(-1).tolist() == [0, 0, 255]


def test_direction_ties_signs_first_and_non_finite():
    w = (1.0, 0.0, 0.0, 0.0)
    z3, z = np.zeros((5, 3), np.float32), np.zeros(5, np.float32)
    c = z3.copy()
    c[:, 0] = [0.5, -0.5, 0.0, float("nan"), float("inf")]
    dev, best, row_dir, imp = A.direction_ref(c, z, z3, z, w, True, None)
    assert dev[:3].tolist() == [0.5, -0.5, 0.0] and math.isnan(dev[3]) and math.isinf(dev[4])
    assert row_dir.tolist() == [1.0, -1.0, 1.0, 1.0, 1.0]           # 0 and non-finite: +1
    assert imp.tolist() == [1, 1, 1, 0, 0]                          # non-finite never improves
    assert best.tolist() == [0.5, -0.5, 0.0, 0.0, 0.0]
    # not first: strictly larger magnitude only; sign does not matter; ties keep the earlier one
    prev = np.array([0.5, 0.4, 0.0, 0.0, 3.0], np.float32)
    c[:, 0] = [-0.5, -0.5, -0.0, 1e-30, float("-inf")]
    dev, best, row_dir, imp = A.direction_ref(c, z, z3, z, w, False, prev)
    assert imp.tolist() == [0, 1, 0, 1, 0]
    assert best.tolist() == [0.5, -0.5, 0.0, np.float32(1e-30), 3.0]
    assert row_dir.tolist() == [-1.0, -1.0, 1.0, 1.0, 1.0]          # -0 >= 0
    # the association is the stated one
    c = np.array([[1e8, 1.0, -1e8]], np.float32)
    s = np.array([0.5], np.float32)
    dev = A.direction_ref(c, s, z3[:1], z[:1], (1.0, 1.0, 1.0, 1.0), True, None)[0]
    assert dev[0] == (np.float32(1e8) + np.float32(1.0)) + (np.float32(-1e8) + np.float32(0.5))


def test_the_draw_is_the_first_24_bit_field():
    u = A.draw_u(0x1234, (2, 3, 4, 5))
    assert u.dtype == np.float32 and u.min() > 0 and u.max() <= 1.0
    h = A.splitmix64(np.uint64((0x1234 + 7 * 0xD1B54A32D192ED03) & A.M64))
    assert u.reshape(-1)[7] == np.float32((int(h) >> 40) + 1) * np.float32(2.0 ** -24)
    assert np.array_equal(A.draw_u(0x1234, (2, 3, 4, 5), np.float64), u.astype(np.float64))
    assert not np.array_equal(A.draw_u(0x1235, (2, 3, 4, 5)), u)


# ---- TrainConfig -------------------------------------------------------------------------------------
def test_defaults_are_todays_config():
    from cilrs_mi355 import CONFIG_A, CONFIG_B, TrainConfig
    from cilrs_mi355.checkpoint import _config_dict
    from cilrs_mi355.train import adv_alpha, check_optim_config
    for cfg in (CONFIG_A, CONFIG_B, TrainConfig()):
        assert cfg.adv_eps == 0.0 and cfg.adv_alpha is None and cfg.adv_random_start is True
        assert cfg.adv_every == 1 and cfg.adv_clamp is False
        check_optim_config(cfg)
    assert TrainConfig() == CONFIG_A and TrainConfig(adv_eps=2.0) != TrainConfig()
    keys = set(_config_dict(types.SimpleNamespace(cfg=CONFIG_A)))
    assert not any(k.startswith("adv_") for k in keys)
    d = _config_dict(types.SimpleNamespace(cfg=TrainConfig(adv_eps=2.0, adv_every=3)))
    assert set(d) == keys | {"adv_eps", "adv_every"} and d["adv_eps"] == 2.0
    assert adv_alpha(TrainConfig(adv_eps=2.0)) == 2.5
    assert adv_alpha(TrainConfig(adv_eps=2.0, adv_random_start=False)) == 2.0
    assert adv_alpha(TrainConfig(adv_eps=2.0, adv_alpha=0.75)) == 0.75


BAD = [
    (dict(adv_eps=-1.0), "adv_eps"),
    (dict(adv_eps=float("nan")), "adv_eps"),
    (dict(adv_eps=float("inf")), "adv_eps"),
    (dict(adv_eps="2"), "adv_eps"),
    (dict(adv_eps=2.0, adv_alpha=-0.5), "adv_alpha"),
    (dict(adv_eps=2.0, adv_alpha=float("nan")), "adv_alpha"),
    (dict(adv_eps=2.0, adv_every=0), "adv_every"),
    (dict(adv_every=1.5), "adv_every"),
    (dict(adv_every=True), "adv_every"),
    (dict(adv_random_start=1), "adv_random_start"),
    (dict(adv_clamp="yes"), "adv_clamp"),
    (dict(adv_eps=2.0, sam_rho=0.05), "sam_rho"),
]


@pytest.mark.parametrize("kw,needle", BAD)
def test_bad_adversarial_options_are_refused_before_anything_is_built(kw, needle):
    from cilrs_mi355 import TrainConfig, Trainer
    from cilrs_mi355.train import check_optim_config

    class Untouchable:
        def engine(self):
            raise AssertionError("the model was touched before the config was checked")

    with pytest.raises(ValueError, match=needle):
        check_optim_config(TrainConfig(**kw))
    with pytest.raises(ValueError, match=needle):
        Trainer(Untouchable(), TrainConfig(**kw))


def test_a_fine_tuning_cut_and_a_bf16_plan_are_refused_at_step_time():
    from cilrs_mi355 import Trainer
    tr = Trainer.__new__(Trainer)
    tr.eng = types.SimpleNamespace(train_precision="fp32")
    tr._refuse_unserved_adversarial(0, 0)
    with pytest.raises(RuntimeError, match="image gradient stops at the cut"):
        tr._refuse_unserved_adversarial(0, 2)
    with pytest.raises(RuntimeError, match="image gradient stops at the cut"):
        tr._refuse_unserved_adversarial(2, 2)
    tr.eng.train_precision = "bf16"
    with pytest.raises(RuntimeError, match="fp32 plans only"):
        tr._refuse_unserved_adversarial(0, 0)


def test_the_adv_every_schedule_and_seeds():
    from cilrs_mi355.train import adv_seed, adv_step_due
    assert [t for t in range(1, 11) if adv_step_due(1, t)] == list(range(1, 11))
    assert [t for t in range(1, 11) if adv_step_due(2, t)] == [1, 3, 5, 7, 9]
    assert [t for t in range(1, 11) if adv_step_due(3, t)] == [1, 4, 7, 10]
    seeds = {adv_seed(1234, k, r) for k in range(1, 50) for r in range(4)}
    assert len(seeds) == 49 * 4 and all(0 <= s < 1 << 64 for s in seeds)


# ---- Predictor.adversarial's own arguments --------------------------------------------------------
def test_default_alpha_and_random_start_rules():
    from cilrs_mi355.adversarial import (CHAN_SCALE, GOALS, RANGE6, attack_args, default_alpha,
                                         default_random_start)
    assert default_alpha(2.0, 1) == 2.0                              # FGSM
    assert default_alpha(2.0, 10) == 0.5 and default_alpha(4.0, 5) == 2.0
    assert [default_random_start(g) for g in GOALS] == [True, False, False, False]
    assert attack_args(2.0, 10, None, None, "deviate", 0) == (2.0, 10, 0.5, True, "deviate", 0)
    assert attack_args(2, 1, None, None, "increase", 7) == (2.0, 1, 2.0, False, "increase", 7)
    assert attack_args(2.0, 3, 0.25, True, "error", 1) == (2.0, 3, 0.25, True, "error", 1)
    for bad in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps="2"), dict(steps=0),
                dict(steps=2.5), dict(alpha=-0.1), dict(alpha=float("inf")), dict(goal="untargeted"),
                dict(random_start="yes"), dict(seed=-1), dict(seed=1 << 64)):
        kw = dict(eps=2.0, steps=10, alpha=None, random_start=None, goal="deviate", seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            attack_args(**kw)
    assert CHAN_SCALE == A.CHAN_SCALE and RANGE6 == A.RANGE6      # the tests' statement is the code's


# ---- the C ABI without a device --------------------------------------------------------------------
def test_refusals_that_need_no_device():
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    assert lib.cilrs_adv_max_elements() == 1 << 30
    assert lib.cilrs_adv_quantize_threads() == 1024
    cs = (C.c_float * 3)(*A.CHAN_SCALE)
    w4 = (C.c_float * 4)(1, 0, 0, 0)
    p = C.c_void_p(4096)                             # never dereferenced: every call is refused
    B, H, W = 2, 4, 6
    st = (3 * H * W, H * W, W, 1)
    nan, inf = float("nan"), float("inf")

    def refused(rc, what):
        assert rc != 0
        msg = lib.cilrs_last_error()
        assert msg and what.encode() in msg, (what, msg)

    start = lib.cilrs_adv_start
    refused(start(None, *st, B, H, W, 1.0, cs, 0, None, p, *st, None), "NULL")
    refused(start(p, *st, B, H, W, 1.0, cs, 0, None, None, *st, None), "NULL")
    refused(start(p, *st, B, H, W, 1.0, None, 0, None, p, *st, None), "NULL")
    for bad in (-1.0, nan, inf):
        refused(start(p, *st, B, H, W, bad, cs, 0, None, p, *st, None), "eps255")
    refused(start(p, st[0], st[1], -st[2], st[3], B, H, W, 1.0, cs, 0, None, p, *st, None),
            "negative stride")
    refused(start(p, *st, B, H, W, 1.0, cs, 0, None, p, st[0], -1, st[2], st[3], None),
            "negative stride")
    refused(start(p, *st, 0, H, W, 1.0, cs, 0, None, p, *st, None), "bad shape")
    refused(start(p, *st, 1 << 15, 1 << 8, 1 << 8, 1.0, cs, 0, None, p, *st, None), "2^30")
    step = lib.cilrs_adv_step
    z = (0, 0, 0, 0)
    refused(step(None, p, *st, p, *st, B, H, W, 1.0, 1.0, cs, None, None, None, *z, None, None), "NULL")
    refused(step(p, None, *st, p, *st, B, H, W, 1.0, 1.0, cs, None, None, None, *z, None, None), "NULL")
    refused(step(p, p, *st, None, *z, B, H, W, 1.0, 1.0, cs, None, None, None, *z, None, None),
            "only when alpha255 = 0")
    for bad in (-1.0, nan, inf):
        refused(step(p, p, *st, p, *st, B, H, W, bad, 1.0, cs, None, None, None, *z, None, None),
                "alpha255")
        refused(step(p, p, *st, p, *st, B, H, W, 1.0, bad, cs, None, None, None, *z, None, None),
                "eps255")
    refused(step(p, p, *st, p, -1, 1, 1, 1, B, H, W, 1.0, 1.0, cs, None, None, None, *z, None, None),
            "negative stride")
    refused(step(p, p, *st, p, *st, B, H, W, 0.0, 1.0, cs, None, p, p, 1, 1, -1, 1, None, None),
            "negative stride")
    refused(step(p, p, *st, p, *st, 1 << 10, 1 << 10, 1 << 10, 1.0, 1.0, cs, None, None, None, *z,
                 None, None), "2^30")
    # alpha255 = 0 with nothing to copy: nothing to do, nothing launched, accepted
    assert step(p, p, *st, None, *z, B, H, W, 0.0, 1.0, cs, None, None, None, *z, None, None) == 0
    direction = lib.cilrs_adv_direction
    refused(direction(p, p, p, p, None, B, 1, p, p, p, p, None), "NULL")
    refused(direction(p, p, p, p, w4, B, 1, p, p, p, None, None), "NULL")
    refused(direction(p, p, p, p, w4, 0, 1, p, p, p, p, None), "at least 1")
    quant = lib.cilrs_adv_quantize
    refused(quant(None, *st, p, B, H, W, p, None, None), "NULL")
    refused(quant(p, *st, p, B, H, W, None, None, None), "NULL")
    refused(quant(p, *st, None, B, H, W, p, p, None), "needs the clean frames")
    refused(quant(p, st[0], st[1], st[2], -1, p, B, H, W, p, None, None), "negative stride")
    refused(quant(p, *st, p, B, -3, W, p, None, None), "bad shape")
