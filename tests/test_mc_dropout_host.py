"""The CPU statement of Monte-Carlo dropout through the heads (tests/_mc_dropout.py) checked against
what the repository already states -- the documented hash (test_ops_edges_gpu.np_keep) and the
oracle's eval forward -- and shown to be sensitive to the mistakes the GPU gates must catch: a wrong
Dropout site, a row taken as s * B + b, a biased standard deviation."""
import numpy as np
import pytest
import torch

import _mc_dropout as D
import test_ops_edges_gpu as E

SEED = 0x51F15EED
B, S, P = 3, 6, 0.5


@pytest.fixture(scope="module")
def case():
    hm = D.build_heads(4, 512)
    v, spd = D.synthetic_features(B, 512)
    cmd = torch.tensor([2, 0, 3], dtype=torch.int64)
    ref = D.mc_samples(hm, v, spd, cmd, S, P, SEED)
    return hm, v, spd, cmd, ref


def _gate(ref):
    return D.TOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("site,cols", [(0, 128), (3, 256), (9, 256), (13, 256), (17, 256)])
@pytest.mark.parametrize("p", [0.5, 0.25])
def test_masks_equal_the_documented_hash(site, cols, p):
    rows = 37
    assert np.array_equal(D.keep(SEED, site, rows, cols, p), E.np_keep(SEED, site, rows, cols, p))
    assert np.array_equal(D.hash_u(SEED, site, 1000), E.np_hash_u(SEED, site, 1000))
    frac = D.keep(SEED, site, rows, cols, p).mean()
    assert abs(frac - (1.0 - p)) < 0.03


def test_sites_follow_the_number_of_commands():
    import cilrs_oracle as O
    assert D.sites(4) == O.DROPOUT_SITES
    assert D.sites(2)["speed_predictor"] == (5,)
    assert D.sites(6)["speed_predictor"] == (13,) and D.sites(6)["control_branches.5"] == (11, 12)
    used = [s for v in D.sites(8).values() for s in v]
    assert sorted(used) == list(range(18))


def test_p_zero_is_the_eval_forward_on_every_sample(case):
    hm, v, spd, cmd, _ = case
    got = D.mc_samples(hm, v, spd, cmd, S, 0.0, SEED)
    want = D.eval_outputs(hm, v, spd, cmd)
    for s in range(S):                                # (float64 GEMMs of different batch sizes)
        assert float((got[:, s] - want).abs().max()) < 1e-12
    mean, std = D.stats64(want.float().unsqueeze(1).expand(B, S, 4))
    assert torch.equal(std, torch.zeros_like(std))
    assert torch.equal(mean, want.float().double())


def test_p_zero_matches_the_full_oracle_forward():
    """the helper's head wiring against CILRSOracle.forward itself (trunk included), float64"""
    import cilrs_oracle as O
    orc = O.build_oracle(0).double().eval()
    img, spd, cmd, _, _ = O.synthetic_batch(2, seed=9, h=33, w=40)
    with torch.no_grad():
        pooled = orc.visual_encoder(img.double())
        c, ps = orc(img.double(), spd.double(), cmd)
    got = D.mc_samples(orc, pooled, spd, cmd, 2, 0.0, SEED)
    want = torch.cat([c, ps.unsqueeze(1)], dim=1)
    assert float((got[:, 0] - want).abs().max()) < 1e-12
    assert float((got[:, 0] - got[:, 1]).abs().max()) < 1e-12


def test_masks_matter_and_fp32_realisation_is_close(case):
    hm, v, spd, cmd, ref = case
    spread = ref.std(dim=1)
    assert float(spread.min()) > 0.05, spread                   # every output moves with the masks
    got32 = D.mc_samples(hm, v, spd, cmd, S, P, SEED, dtype=torch.float32)
    err = float((got32.double() - ref).abs().max())
    print(f"MC host: fp32 realisation {err:.3g} from float64, max|ref| {float(ref.abs().max()):.3g}, "
          f"std over samples {float(spread.min()):.3g} .. {float(spread.max()):.3g}")
    assert err < _gate(ref) / 4


def test_sensitive_to_a_wrong_site(case):
    hm, v, spd, cmd, ref = case

    def shifted(nc):                                  # the speed predictor on the reference's 9
        st = dict(D.sites(nc))
        st["speed_predictor"] = (2 * nc + 2,)
        return st

    def swapped(nc):                                  # a branch's two sites exchanged
        st = dict(D.sites(nc))
        for k in range(nc):
            a, b = st[f"control_branches.{k}"]
            st[f"control_branches.{k}"] = (b, a)
        return st

    for fn, cols in ((shifted, [3]), (swapped, [0, 1, 2])):
        got = D.mc_samples(hm, v, spd, cmd, S, P, SEED, sites_fn=fn)
        moved = float((got - ref)[..., cols].abs().max())
        assert moved > 1000 * _gate(ref), (fn.__name__, moved)


def test_sensitive_to_the_row_rule(case):
    hm, v, spd, cmd, ref = case
    got = D.mc_samples(hm, v, spd, cmd, S, P, SEED, row_fn=lambda b, s, nb, ns: s * nb + b)
    assert float((got[0, 0] - ref[0, 0]).abs().max()) < 1e-12   # row 0 is row 0 under both rules
    assert float((got - ref).abs().max()) > 1000 * _gate(ref)


def test_sensitive_to_a_biased_std(case):
    *_, ref = case
    smp = ref.float()
    mean, std = D.stats64(smp)
    mean_b, std_b = D.stats64(smp, unbiased=False)
    assert torch.equal(mean, mean_b)
    rel = float(((std - std_b).abs() / std).min())
    assert rel > 1000 * D.TOL_STATS, rel                        # sqrt(S / (S - 1)) - 1 = 9.5e-2 at S = 6
    want = smp.double().std(dim=1)                              # torch's default: unbiased
    assert float((std - want).abs().max()) < 1e-12
    assert float((mean - smp.double().mean(dim=1)).abs().max()) < 1e-12


def test_statistics_of_equal_samples_are_exact():
    x = torch.tensor([0.1, -2.7182817, 3.0e-5, 91.25], dtype=torch.float32)
    for n in (1, 2, 33, 4096):
        mean, std = D.stats64(x.view(1, 1, 4).expand(1, n, 4))
        assert torch.equal(mean[0], x.double()), n
        assert torch.equal(std, torch.zeros(1, 4, dtype=torch.float64)), n
