"""Prioritised sampling without a device: the definition of tests/_priority.py is a sampler (range,
tiling, distribution), and the Python layer's refusals, state round trip and view= refusal.

The distribution check: over R = 2,000 draws of B = 128 with fixed seeds the count of bin i is a sum
of R * B indicator draws with mean R * B * q_i / total and, unstratified, variance R * B * p (1 - p)
(stratified draws of one batch are negatively correlated across its slices, so the variance is no
larger).  Every bin whose expectation exceeds 5 has to lie within 6 of those standard deviations;
the streams are fixed, so the test is deterministic."""
import numpy as np
import pytest
import torch

import _priority as P


def test_single_entry_table_total_below_batch():
    q = np.array([1], dtype=np.uint32)            # total = 1 < B = 8: the unstratified branch
    for stratified in (True, False):
        pos, index, w = P.draw(q, 8, seed=3, counter=0, stratified=stratified, beta=0.4)
        assert pos.tolist() == [0] * 8 and index.tolist() == [0] * 8
        assert w.tolist() == [1.0] * 8


@pytest.mark.parametrize("total,batch", [(8, 8), (9, 8), (1000, 7), (2 ** 40 + 5, 128),
                                          (2 ** 62 + 1023, 1024)])
def test_segments_tile_the_total(total, batch):
    seg = P.segments(total, batch)
    at = 0
    for lo, ln in seg:
        assert lo == at and ln >= 1
        at += ln
    assert at == total
    for t, (lo, ln) in zip(P.targets(total, batch, 11, 5, True), seg):
        assert lo <= t < lo + ln


def _tables():
    five = np.array([7, 1, P.Q_MAX, 1 << 20, 3], dtype=np.uint32)
    rng = np.random.default_rng(1025)
    big = rng.integers(1, 1 << 24, size=1025, dtype=np.uint64).astype(np.uint32)
    return {"n5": five, "n1025": big}


@pytest.mark.parametrize("name", ["n5", "n1025"])
@pytest.mark.parametrize("stratified", [True, False])
def test_draw_follows_the_table(name, stratified):
    q = _tables()[name]
    R, B = 2000, 128
    cum = np.cumsum(q.astype(np.uint64), dtype=np.uint64)
    counts = np.zeros(len(q), dtype=np.int64)
    for c in range(R):
        pos, _, _ = P.draw(q, B, seed=20240607, counter=c, stratified=stratified, beta=0.0, cum=cum)
        assert pos.min() >= 0 and pos.max() < len(q)
        counts += np.bincount(pos, minlength=len(q))
    p = q.astype(np.float64) / float(int(cum[-1]))
    mean = R * B * p
    sd = np.sqrt(R * B * p * (1.0 - p))
    live = mean > 5
    assert live.any()
    z = np.abs(counts[live] - mean[live]) / np.maximum(sd[live], 1e-300)
    print(f"{name} stratified={stratified}: max |z| = {z.max():.2f} over {int(live.sum())} bins")
    assert z.max() <= 6.0
    assert counts.sum() == R * B


def test_update_definition_rules():
    q = P.fill(None, 4)
    assert q.tolist() == [P.FIXED_ONE] * 4
    q2, pmax = P.update(q, [1, 1, 9, -1, 3], np.array([1.0, 3.0, 5.0, 5.0, np.inf], np.float32),
                        None, 1.0, 0.5, P.FIXED_ONE)
    assert q2.tolist() == [P.FIXED_ONE, int(3.5 * P.FIXED_ONE), P.FIXED_ONE, P.Q_MAX]
    assert pmax == P.Q_MAX
    assert P.fixed(float("nan")) == P.Q_MAX and P.fixed(0.0) == 1 and P.fixed(1e300) == P.Q_MAX


# ---- the Python layer --------------------------------------------------------------------------------
def _sampler(**kw):
    from cilrs_mi355 import PrioritySampler
    args = dict(n=6, device="cpu")
    args.update(kw)
    return PrioritySampler(**args)


@pytest.mark.parametrize("kw,word", [
    (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"),
    (dict(beta=-0.01), "beta"), (dict(beta=1.01), "beta"),
    (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"),
    (dict(base=[1, 1, 1, 0, 1, 1]), "base"), (dict(base=[1, 1, 1, float("inf"), 1, 1]), "base"),
    (dict(base=[1, 1, 1, float("nan"), 1, 1]), "base"), (dict(base=[1.0] * 5), "base"),
    (dict(subset=[0, 1, 2, 3, 4, 10], n_frames=10), "subset"),
    (dict(subset=[0, 1, 2, 3, 4, -1], n_frames=10), "subset"),
    (dict(subset=[0, 1, 2, 3, 4, 5]), "n_frames"),
    (dict(n=0), "n"), (dict(n=2 ** 31 + 1), "n"),
])
def test_sampler_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        _sampler(**kw)


def test_sampler_accepts_the_edges():
    s = _sampler(alpha=0.0, beta=1.0, eps=1e-12, base=[0.5] * 6, subset=[9, 0, 3, 3, 2, 1],
                 n_frames=10)
    assert s.n == 6 and s.n_frames == 10 and s.counter == 0


def test_no_cpu_fallback():
    s = _sampler()
    with pytest.raises(RuntimeError, match="GPU"):
        s.draw(4)
    with pytest.raises(RuntimeError, match="GPU"):
        s.update(torch.zeros(4, dtype=torch.int64), torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):
        s.fill()


def test_state_dict_round_trip():
    a = _sampler(seed=5)
    q = torch.tensor([1, 2, -1, 1 << 20, 7, 3], dtype=torch.int32)       # -1: the bits of 2^32 - 1
    sd = {"n": 6, "alpha": a.alpha, "beta": a.beta, "eps": a.eps, "stratified": True, "seed": 5,
          "counter": 41, "q": q, "pmax": torch.tensor([1 << 21], dtype=torch.int32)}
    a.load_state_dict(sd)
    out = a.state_dict()
    assert out["counter"] == 41 and torch.equal(out["q"], q) and int(out["pmax"][0]) == 1 << 21
    assert a.table().tolist() == [1, 2, P.Q_MAX, 1 << 20, 7, 3]
    assert a.running_max() == 1 << 21
    np.testing.assert_allclose(a.probabilities().sum().item(), 1.0, rtol=1e-12)
    b = _sampler(seed=5)
    b.load_state_dict(out)
    assert b.counter == 41 and torch.equal(b.state_dict()["q"], q)
    out["q"][0] = 99                              # a copy, not the live table
    assert b.table()[0] == 1
    with pytest.raises(ValueError, match="seed"):
        _sampler(seed=6).load_state_dict(sd)
    with pytest.raises(ValueError, match="entries"):
        _sampler(n=7).load_state_dict(sd)
    bad = dict(sd, q=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="zeros"):
        _sampler(seed=5).load_state_dict(bad)


class _FakeDataset:
    device = torch.device("cpu")
    h, w, filled = 88, 200, False
    command = np.array([0, 1, 2, 3] * 8)

    def __len__(self):
        return 32


def test_loader_refuses_view_and_counts_batches():
    from cilrs_mi355 import PrioritizedBatchLoader, ViewShift
    ds = _FakeDataset()
    with pytest.raises(ValueError, match="view="):
        PrioritizedBatchLoader(ds, np.arange(32), 8, view=ViewShift())
    ld = PrioritizedBatchLoader(ds, np.arange(2, 32), 8)
    assert len(ld) == 30 // 8
    assert ld.sampler.n == 30 and ld.sampler.n_frames == 32
    with pytest.raises(RuntimeError, match="before the first batch"):
        ld.feedback(torch.zeros(8))
    with pytest.raises(ValueError, match="rank"):
        PrioritizedBatchLoader(ds, np.arange(32), 8, rank=2, world_size=2)
    two = PrioritizedBatchLoader(ds, np.arange(32), 4, rank=1, world_size=2)
    assert two.sampler.n == 16 and len(two) == 4
    with pytest.raises(ValueError, match="alpha"):
        PrioritizedBatchLoader(ds, np.arange(32), 8, alpha=-1.0)


def test_train_step_signature_keeps_the_plain_call():
    import inspect
    from cilrs_mi355 import Trainer
    sig = inspect.signature(Trainer.train_step)
    assert list(sig.parameters)[:5] == ["self", "imgs", "speeds", "cmds", "tgts"]
    assert sig.parameters["sample_weight"].default is None
    assert sig.parameters["row_loss"].default is None
