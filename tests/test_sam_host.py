"""Sharpness-aware minimisation, host side: the two CPU statements of tests/_sam.py against each
other and on their identities, the TrainConfig refusals before anything is built, the sam_every
schedule, the defaults, the checkpoint config keys and the size queries of the C ABI."""
import math
import types

import pytest
import torch

import _optim as Q
import _sam as S


def _data(n, seed, p_scale=0.05, g_scale=1e-3):
    gen = torch.Generator().manual_seed(seed)
    p = p_scale * torch.randn(n, generator=gen)
    g = g_scale * torch.randn(n, generator=gen) * 10.0 ** torch.randint(-3, 2, (n,), generator=gen).float()
    return p, g


@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("rho", [0.05, 2.0])
def test_the_fp32_statement_is_within_fp32_rounding_of_the_float64_one(adaptive, rho):
    p, g = _data(10_000, 3)
    want, s_sum, norm, scale = S.perturb64(p, g, rho, adaptive)
    assert s_sum > 0 and norm == math.sqrt(s_sum) and scale == rho / (norm + 1e-12)
    got = S.perturb32(p, g, S.s32_of(scale), adaptive)
    # per element: (float)scale, the product chain (up to three roundings, relative to the step) and
    # the final sum (relative to the result): (1 + 3 + 1) * 2^-24 of |step| plus 2^-24 of |p_new|
    step = (want - p.double()).abs()
    bound = 2.0 ** -24 * (5.0 * step + want.abs()) + 1e-45
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert not torch.equal(got, p)
    # |e| = rho for plain SAM, to the rounding of the elements
    if not adaptive:
        assert float((want - p.double()).norm()) == pytest.approx(rho, rel=1e-9)
    Q.gate("perturb32 as its own device", got, want, got)


@pytest.mark.parametrize("adaptive", [0, 1])
def test_identities_of_the_definition(adaptive):
    p, g = _data(4096, 5)
    p[::7] = 0.0
    # rho = 0: the scale is zero
    want, _, _, scale = S.perturb64(p, g, 0.0, adaptive)
    assert scale == 0.0 and torch.equal(want, p.double())
    assert torch.equal(S.perturb32(p, g, 0.0, adaptive), p)
    # g = 0: S = 0, scale = rho * 1e12, times zero
    z = torch.zeros_like(g)
    want, s_sum, norm, scale = S.perturb64(p, z, 0.05, adaptive)
    assert s_sum == 0.0 and norm == 0.0 and scale == 0.05 / 1e-12
    assert torch.equal(want, p.double())
    out = S.perturb32(p, z, S.s32_of(scale), adaptive)
    assert torch.equal(out, p) and bool(torch.isfinite(out).all())
    # the adaptive form leaves zero weights at zero; the plain one moves them
    out = S.perturb32(p, g, S.s32_of(S.perturb64(p, g, 0.05, adaptive)[3]), adaptive)
    moved = bool((out[::7] != 0).any())
    assert moved == (not adaptive)
    # inputs are not modified
    p2, g2 = _data(4096, 5)
    p2[::7] = 0.0
    assert torch.equal(p, p2) and torch.equal(g, g2)


def test_the_adaptive_norm_is_the_norm_of_the_rounded_product():
    p, g = _data(1000, 9)
    t = (p.abs() * g).double()
    assert S.norm_scale(p, g, 0.1, 1)[0] == math.fsum((t * t).tolist())
    assert S.norm_scale(p, g, 0.1, 0)[0] == math.fsum((g.double() ** 2).tolist())
    # ASAM is invariant to rescaling a weight and its gradient inversely (Kwon et al. 2021): e / w is
    assert S.s32_of(1e39) == float("inf") and S.s32_of(0.1) == float(torch.tensor(0.1))
    e1 = S.perturb64(p, g, 0.1, 1)[0] - p.double()
    p4, g4 = p * 4.0, g / 4.0                                   # exact in fp32
    e4 = S.perturb64(p4, g4, 0.1, 1)[0] - p4.double()
    nz = p != 0
    assert torch.allclose(e4[nz] / p4.double()[nz], e1[nz] / p.double()[nz], rtol=1e-12, atol=0)


BAD = [
    (dict(sam_rho=-0.1), "sam_rho"),
    (dict(sam_rho=float("nan")), "sam_rho"),
    (dict(sam_rho=float("inf")), "sam_rho"),
    (dict(sam_rho="0.05"), "sam_rho"),
    (dict(sam_rho=0.05, sam_every=0), "sam_every"),
    (dict(sam_every=-2), "sam_every"),
    (dict(sam_every=1.5), "sam_every"),
]


@pytest.mark.parametrize("kw,needle", BAD)
def test_bad_sam_options_are_refused_before_anything_is_built(kw, needle):
    from cilrs_mi355 import TrainConfig, Trainer
    from cilrs_mi355.train import check_optim_config

    class Untouchable:
        def engine(self):
            raise AssertionError("the model was touched before the config was checked")

    with pytest.raises(ValueError, match=needle):
        check_optim_config(TrainConfig(**kw))
    with pytest.raises(ValueError, match=needle):
        Trainer(Untouchable(), TrainConfig(**kw))


def test_fuse_optimizer_with_sam_is_refused_at_step_time_in_the_existing_style():
    from cilrs_mi355 import TrainConfig, Trainer
    from cilrs_mi355.train import check_optim_config
    cfg = TrainConfig(sam_rho=0.05)
    check_optim_config(cfg)                                      # the config itself is fine
    tr = Trainer.__new__(Trainer)
    tr.cfg, tr.fuse_optimizer, tr.ema_fused = cfg, True, False
    with pytest.raises(RuntimeError, match=r"Trainer\.fuse_optimizer cannot serve sam_rho"):
        tr._refuse_unserved_optimizer()
    tr.fuse_optimizer = False
    tr._refuse_unserved_optimizer()
    tr.cfg, tr.fuse_optimizer = TrainConfig(), True              # SAM off: nothing new is refused
    tr._refuse_unserved_optimizer()


def test_the_sam_every_schedule():
    from cilrs_mi355.train import sam_step_due
    assert [t for t in range(1, 11) if sam_step_due(1, t)] == list(range(1, 11))
    assert [t for t in range(1, 11) if sam_step_due(2, t)] == [1, 3, 5, 7, 9]
    assert [t for t in range(1, 11) if sam_step_due(3, t)] == [1, 4, 7, 10]
    assert [t for t in range(1, 30) if sam_step_due(10, t)] == [1, 11, 21]
    for k in (1, 2, 5):
        assert all(sam_step_due(k, t) == ((t - 1) % k == 0) for t in range(1, 50))


def test_defaults_are_todays_config():
    from cilrs_mi355 import CONFIG_A, CONFIG_B, TrainConfig
    from cilrs_mi355.checkpoint import _config_dict
    for cfg in (CONFIG_A, CONFIG_B, TrainConfig()):
        assert cfg.sam_rho == 0.0 and cfg.sam_adaptive is False and cfg.sam_every == 1
    assert TrainConfig() == CONFIG_A == TrainConfig(sam_rho=0.0, sam_adaptive=False, sam_every=1)
    assert TrainConfig(sam_rho=0.05) != TrainConfig()
    # a checkpoint written with SAM off has the keys it always had; set fields are recorded
    keys = set(_config_dict(types.SimpleNamespace(cfg=CONFIG_A)))
    assert not any(k.startswith("sam_") for k in keys)
    d = _config_dict(types.SimpleNamespace(cfg=TrainConfig(sam_rho=0.05, sam_every=2)))
    assert set(d) == keys | {"sam_rho", "sam_every"} and d["sam_rho"] == 0.05 and d["sam_every"] == 2


def test_size_queries_and_refusals_that_need_no_device():
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    chunk = lib.cilrs_sam_chunk_floats()
    assert chunk == 4096
    for n, chunks in ((4, 1), (chunk - 4, 1), (chunk, 1), (chunk + 4, 2), (3 * chunk + 12, 4),
                      (1_048_580, 257), (22_421_460, 5474)):
        want = (chunks + 3) * 8
        assert lib.cilrs_sam_scratch_bytes(n) == (want + 15) // 16 * 16, n
    assert lib.cilrs_sam_scratch_bytes(0) == 0 and lib.cilrs_sam_scratch_bytes(2 ** 30 + 4) == 0
    # the longest run of sequential additions: 16 per thread in a chunk, chunks / 256 in the finalise
    assert chunk // 4 // 256 * 4 == 16 and (2 ** 30 // chunk) // 256 == 1024
    # refused on the host: nothing below reaches a launch (no device here)
    assert lib.cilrs_sam_perturb(None, None, None, 4, 0.05, 0, None, None, None) != 0
    assert b"NULL" in lib.cilrs_last_error()
    assert lib.cilrs_sam_restore(None, None, 4, None) != 0
    assert b"NULL" in lib.cilrs_last_error()
