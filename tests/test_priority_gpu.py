"""Prioritised sampling on the device against the definition of tests/_priority.py: the per-sample
loss entry (bit-equal to cilrs_loss_fwd_bwd without weights, float64 autograd with them), the
fixed-point update, the draw (positions and indices exactly, weights to 1e-6), and the loader /
Trainer / loop path end to end.

Bounds.  Row losses: the device forms l_b in double from the fp32 differences and rounds once; the
definition does the same without fused multiply-adds, so the two doubles agree to a few 2^-53 and
the fp32 values to one rounding.  Weighted gradients: an fp32 difference, a division or product by
the batch constants and the product by the weight, each within 2^-24 relative -- under 3e-7 against
float64, held to 1e-6; the terms are double sums of fewer than 1,000 non-negative addends of such
values, held to 1e-6 too.  Update: alpha in {0, 0.5, 1} is 1, sqrt and the value itself, exactly
rounded on both sides; any other alpha goes through pow, which is not numpy's bit for bit, so the
entry may differ by max(1, q * 2^-20) counts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _priority as P
import cilrs_oracle as O
from _guards import Inputs, guarded

pytestmark = pytest.mark.gpu

W4 = {0: (1.0, 1.0, 1.0, 0.05), 1: (5.0, 1.0, 1.0, 0.5)}


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gbuf(cpu, name):
    v, check = guarded(cpu.numel(), dtype=cpu.dtype, fill=None, name=name)
    v.copy_(cpu.reshape(-1))
    return v, check


def bits(a):
    """numpy uint32 -> the int32 tensor that carries the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy())


def unbits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


# ---- rows entry ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_data(B):
    g = torch.Generator().manual_seed(77 + B)
    pc, tc = torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)
    ps, ts = torch.rand(B, generator=g), torch.rand(B, generator=g)
    tc[0, 1] = pc[0, 1]                       # sign(0) and a zero square
    if B > 2:
        ts[2] = ps[2]
    w = torch.rand(B, generator=g) * 1.5 + 0.01
    return pc, tc, ps, ts, w


class LossCall:
    def __init__(self, B, kind, rows, weight=None, want_rows=True):
        L = _L()
        pc, tc, ps, ts, _ = loss_data(B)
        self.pc, self.tc, self.ps, self.ts = pc.cuda(), tc.cuda(), ps.cuda(), ts.cuda()
        self.w = None if weight is None else weight.cuda()
        self.dc, c1 = guarded(B * 3, name="dcontrols")
        self.dp, c2 = guarded(B, name="dpred_speed")
        self.out, c3 = guarded(6, name="loss_out")
        self.rl, c4 = guarded(B, name="row_loss")
        ins = Inputs(pc=self.pc, tc=self.tc, ps=self.ps, ts=self.ts, w=self.w)
        w4 = (C.c_float * 4)(*W4[kind])
        if rows:
            L.check(L.lib().cilrs_loss_fwd_bwd_rows(
                L.ptr(self.pc), L.ptr(self.tc), L.ptr(self.ps), L.ptr(self.ts), B, kind, w4, 1.0,
                L.ptr(self.dc), L.ptr(self.dp), L.ptr(self.out), L.ptr(self.w),
                L.ptr(self.rl) if want_rows else None, stream()))
        else:
            L.check(L.lib().cilrs_loss_fwd_bwd(
                L.ptr(self.pc), L.ptr(self.tc), L.ptr(self.ps), L.ptr(self.ts), B, kind, w4, 1.0,
                L.ptr(self.dc), L.ptr(self.dp), L.ptr(self.out), stream()))
        for c in (c1, c2, c3, c4):
            c()
        ins.check()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 256, 257])
def test_rows_entry_without_weights_is_the_plain_loss(B, kind):
    plain = LossCall(B, kind, rows=False)
    rows = LossCall(B, kind, rows=True)
    for name in ("out", "dc", "dp"):
        assert torch.equal(getattr(plain, name), getattr(rows, name)), name
    assert torch.isnan(plain.rl).all()                         # the plain entry writes none
    pc, tc, ps, ts, _ = loss_data(B)
    want = P.loss_rows(pc.numpy(), tc.numpy(), ps.numpy(), ts.numpy(), kind, W4[kind])
    got = rows.rl.cpu().numpy()
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print(f"B={B} kind={kind}: row_loss max error {float((err / ulp).max()):.2f} ulp")
    assert (err <= ulp).all()
    # the mean of the rows is the total
    np.testing.assert_allclose(want.mean(), float(rows.out[0]), rtol=1e-6)
    # all-ones weights: the same bits again; no row_loss asked for: nothing written there
    ones = LossCall(B, kind, rows=True, weight=torch.ones(B), want_rows=False)
    for name in ("out", "dc", "dp"):
        assert torch.equal(getattr(plain, name), getattr(ones, name)), name
    assert torch.isnan(ones.rl).all()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 256, 257])
def test_rows_entry_with_weights_against_float64_autograd(B, kind):
    pc, tc, ps, ts, w = loss_data(B)
    call = LossCall(B, kind, rows=True, weight=w)
    pcd = pc.double().requires_grad_(True)
    psd = ps.double().requires_grad_(True)
    wd, w4 = w.double(), W4[kind]
    d, ds = pcd - tc.double(), psd - ts.double()
    per = (d * d if kind == 0 else d.abs()) * wd[:, None]
    chan = per.mean(0)                                          # (1 / B) sum_b w_b term
    speed = (wd * ds * ds).mean()
    control = chan.mean() if kind == 0 else w4[0] * chan[0] + w4[1] * chan[1] + w4[2] * chan[2]
    total = control + w4[3] * speed
    total.backward()
    want = torch.stack([total, control, chan[0], chan[1], chan[2], speed]).detach()
    got = call.out.cpu().double()
    te = (got - want).abs()
    gd = (call.dc.cpu().double().view(B, 3) - pcd.grad).abs()
    gs = (call.dp.cpu().double() - psd.grad).abs()
    print(f"B={B} kind={kind}: terms {float((te / want.abs().clamp_min(1e-300)).max()):.2e}, "
          f"dcontrols {float((gd / pcd.grad.abs().clamp_min(1e-300)).max()):.2e}, "
          f"dspeed {float((gs / psd.grad.abs().clamp_min(1e-300)).max()):.2e} relative")
    assert bool((te <= 1e-6 * want.abs()).all())
    assert bool((gd <= 1e-6 * pcd.grad.abs()).all())
    assert bool((gs <= 1e-6 * psd.grad.abs()).all())
    # the rows themselves carry no weight
    rows = P.loss_rows(pc.numpy(), tc.numpy(), ps.numpy(), ts.numpy(), kind, w4)
    np.testing.assert_allclose(call.rl.cpu().numpy(), rows, rtol=2e-7, atol=0)


# ---- update -----------------------------------------------------------------------------------------------
def run_update(q0, pos, loss, base, alpha, eps, pmax0):
    L = _L()
    n = len(q0)
    q, cq = gbuf(bits(q0), "q")
    pm, cp = gbuf(bits(np.array([pmax0], dtype=np.uint32)), "pmax_state")
    pos_d, loss_d = torch.from_numpy(pos).cuda(), torch.from_numpy(loss).cuda()
    base_d = None if base is None else torch.from_numpy(base).cuda()
    ins = Inputs(pos=pos_d, loss=loss_d, base=base_d)
    L.check(L.lib().cilrs_priority_update(L.ptr(q), n, L.ptr(pos_d), L.ptr(loss_d), L.ptr(base_d),
                                          alpha, eps, L.ptr(pm), len(pos), stream()))
    cq()
    cp()
    ins.check()
    return unbits(q), int(unbits(pm)[0])


def update_case(n, B, seed, same=False):
    rng = np.random.default_rng(seed)
    q0 = rng.integers(1, 1 << 22, size=n, dtype=np.uint64).astype(np.uint32)
    pos = rng.integers(0, n, size=B).astype(np.int64)
    if same:
        pos[:] = n // 2
    else:
        pos[rng.integers(0, B, size=3)] = [-1, n, n + 5]          # never written
    loss = (rng.random(B) * 10.0 ** rng.integers(-4, 3, size=B)).astype(np.float32)
    base = (rng.random(n) * 3 + 0.05).astype(np.float32)
    return q0, pos, loss, base


@pytest.mark.parametrize("n", [1, 63, 1025])
def test_update_against_the_definition(n):
    for B, same in ((64, False), (64, True), (1, False), (1024, False)):
        q0, pos, loss, base = update_case(n, B, 100 * n + B, same)
        if B > 1 and n > 1 and not same:
            assert len(set(pos.tolist())) < B                    # positions repeat
        for alpha in (0.0, 0.5, 1.0, 0.6):
            for bs in (base, None):
                got, gmax = run_update(q0, pos, loss, bs, alpha, 1e-3, 1 << 20)
                want, wmax = P.update(q0, pos, loss, bs, alpha, 1e-3, 1 << 20)
                diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
                if alpha == 0.6:
                    tol = np.maximum(1, want.astype(np.float64) * 2.0 ** -20)
                    assert (diff <= tol).all(), (n, B, alpha, int(diff.max()))
                    assert abs(gmax - wmax) <= max(1, wmax * 2.0 ** -20)
                else:
                    assert (diff == 0).all(), (n, B, alpha, int(diff.max()))
                    assert gmax == wmax
                named = np.zeros(n, dtype=bool)
                named[pos[(pos >= 0) & (pos < n)]] = True
                assert (got[~named] == q0[~named]).all()         # bit-unchanged where not named


def test_update_clamps_and_keeps_the_running_maximum():
    n = 63
    q0 = np.full(n, 1 << 20, dtype=np.uint32)
    pos = np.array([0, 1, 2, 3, 4, 5, 5], dtype=np.int64)
    loss = np.array([np.inf, np.nan, -np.inf, 1e30, 0.0, 3.0, 2.0], dtype=np.float32)
    got, gmax = run_update(q0, pos, loss, None, 1.0, 1e-3, 1 << 20)
    assert got[:4].tolist() == [P.Q_MAX] * 4
    assert got[4] == P.fixed(1e-3) and got[5] == P.fixed(float(np.float32(2.0)) + 1e-3)
    assert gmax == P.Q_MAX
    # alpha = 0 does not hide a non-finite loss (pow(nan, 0) is 1)
    got, gmax = run_update(q0, pos[:2], loss[:2], None, 0.0, 1e-3, 1 << 20)
    assert got[:2].tolist() == [P.Q_MAX] * 2
    # nothing above the old maximum: it stays; tiny priorities clamp to 1
    got, gmax = run_update(q0, pos[4:5], np.array([0.0], np.float32), None, 1.0, 1e-9, 1 << 24)
    assert got[4] == 1 and gmax == 1 << 24
    L = _L()
    q = bits(q0).cuda()
    bad = L.lib().cilrs_priority_update(L.ptr(q), n, L.ptr(q), L.ptr(q), None, 0.6, 1e-3, L.ptr(q),
                                        1025, stream())
    assert bad != 0 and b"batch" in L.lib().cilrs_last_error()


def test_fill_is_base_times_the_running_maximum():
    L = _L()
    rng = np.random.default_rng(3)
    n = 1025
    base = (rng.random(n) * 4 + 1e-8).astype(np.float32)
    base[:3] = [1e-9, 5000.0, 1.0]
    for pmax in (1 << 20, 3 << 20):
        q, cq = guarded(n, dtype=torch.int32, fill=0, name="q")
        pm = bits(np.array([pmax], dtype=np.uint32)).cuda()
        L.check(L.lib().cilrs_priority_fill(L.ptr(q), n, L.ptr(torch.from_numpy(base).cuda()),
                                            L.ptr(pm), stream()))
        cq()
        assert (unbits(q) == P.fill(base, n, pmax)).all()
    assert P.fill(base, n)[0] == 1 and P.fill(base, n, 3 << 20)[1] == P.Q_MAX


# ---- draw -------------------------------------------------------------------------------------------------
def draw_tables(n):
    """name -> table: all ones; one entry 2^32 - 1 among ones at the start, the end and either side
    of the first chunk boundary; random"""
    out = {"ones": np.ones(n, dtype=np.uint32)}
    for name, at in (("first", 0), ("last", n - 1), ("chunk_end", P.CHUNK - 1),
                     ("chunk_start", P.CHUNK)):
        if 0 <= at < n and (name in ("first", "last") or n > at):
            t = np.ones(n, dtype=np.uint32)
            t[at] = P.Q_MAX
            out[name] = t
    rng = np.random.default_rng(n)
    out["random"] = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return out


def run_draw(q_d, n, subset_d, n_frames, seed, counter, B, stratified, beta, scratch):
    L = _L()
    pos, c1 = guarded(B, dtype=torch.int64, fill=-7, name="out_pos")
    idx, c2 = guarded(B, dtype=torch.int64, fill=-7, name="out_index")
    wgt, c3 = guarded(B, name="out_weight")
    L.check(L.lib().cilrs_priority_draw(L.ptr(q_d), n, L.ptr(subset_d), n_frames, seed, counter, B,
                                        1 if stratified else 0, beta, L.ptr(pos), L.ptr(idx),
                                        L.ptr(wgt), L.ptr(scratch), stream()))
    for c in (c1, c2, c3):
        c()
    return pos.cpu(), idx.cpu(), wgt.cpu()


@pytest.mark.parametrize("n", [1, 2, 255, 1024, 1025, 4097, 70_001])
def test_draw_against_the_definition(n):
    L = _L()
    nbytes = L.lib().cilrs_priority_scratch_bytes(n)
    assert nbytes == ((n + P.CHUNK - 1) // P.CHUNK + 1) * 8          # sized exactly
    rng = np.random.default_rng(9 + n)
    n_frames = 2 * n + 3
    subset = rng.permutation(n_frames)[:n].astype(np.int64)
    subset_d = torch.from_numpy(subset).cuda()
    seed = 0x9E3779B97F4A7C15 ^ n
    worst = 0.0
    for name, table in draw_tables(n).items():
        q_d, cq = gbuf(bits(table), "q")
        ins = Inputs(q=q_d, subset=subset_d)
        cum = np.cumsum(table.astype(np.uint64), dtype=np.uint64)
        for B in (1, 7, 128, 1024):
            scratch, cs = guarded(nbytes, dtype=torch.uint8, fill=None, name="scratch")
            for k, (stratified, use_subset, counter, beta) in enumerate(
                    [(s, u, c, 0.4) for s in (True, False) for u in (True, False)
                     for c in (0, (1 << 40) + 3)] + [(True, False, 1, 0.0), (False, True, 1, 1.0)]):
                sub = subset if use_subset else None
                got = run_draw(q_d, n, subset_d if use_subset else None,
                               n_frames if use_subset else n, seed, counter, B, stratified, beta,
                               scratch)
                want = P.draw(table, B, seed, counter, stratified, beta, sub, cum=cum)
                tag = (n, name, B, stratified, use_subset, counter, beta)
                assert torch.equal(got[0], torch.from_numpy(want[0])), tag
                assert torch.equal(got[1], torch.from_numpy(want[1])), tag
                w = got[2].numpy().astype(np.float64)
                if beta == 0.0:
                    assert (got[2] == 1.0).all(), tag
                rel = np.abs(w - want[2].astype(np.float64)) / want[2].astype(np.float64)
                worst = max(worst, float(rel.max()))
                assert rel.max() <= 1e-6, tag
                assert w.max() == 1.0 and w.min() > 0.0, tag
                if k == 0:                                        # run to run
                    again = run_draw(q_d, n, subset_d, n_frames, seed, counter, B, stratified,
                                     beta, scratch)
                    assert all(torch.equal(a, b) for a, b in zip(got, again)), tag
            cs()
        cq()
        ins.check()
    print(f"n={n}: weights within {worst:.2e} relative")


def test_draw_refusals():
    L = _L()
    q = torch.ones(64, dtype=torch.int32, device="cuda")
    o = torch.zeros(64, dtype=torch.int64, device="cuda")
    w = torch.zeros(64, device="cuda")
    s = torch.zeros(16, dtype=torch.int64, device="cuda")

    def call(n=64, B=8, beta=0.4, strat=1, qq=q, n_frames=64):
        return L.lib().cilrs_priority_draw(L.ptr(qq), n, None, n_frames, 1, 0, B, strat, beta,
                                           L.ptr(o), L.ptr(o), L.ptr(w), L.ptr(s), stream())
    assert call() == 0
    for kw, word in ((dict(n=0), b"n ="), (dict(B=0), b"batch"), (dict(B=1025), b"batch"),
                     (dict(beta=1.5), b"beta"), (dict(beta=float("nan")), b"beta"),
                     (dict(strat=2), b"stratified"), (dict(qq=q[1:]), b"aligned"),
                     (dict(n_frames=63), b"n_frames")):
        assert call(**kw) != 0 and word in L.lib().cilrs_last_error(), kw
    assert L.lib().cilrs_priority_scratch_bytes(0) == 0
    assert L.lib().cilrs_priority_scratch_bytes((1 << 31) + 1) == 0
    assert L.lib().cilrs_priority_scratch_bytes(1 << 31) == ((1 << 21) + 1) * 8
    assert L.lib().cilrs_priority_max_batch() == 1024
    torch.cuda.synchronize()


def test_sampler_object_matches_the_definition():
    from cilrs_mi355 import PrioritySampler
    n = 1500
    rng = np.random.default_rng(4)
    base = (rng.random(n) + 0.25).astype(np.float32)
    subset = rng.permutation(4000)[:n]
    s = PrioritySampler(n, "cuda", base=base, subset=subset, n_frames=4000, alpha=0.5, beta=0.4,
                        seed=12)
    table = s.table()
    assert (table == P.fill(base, n)).all() and s.running_max() == 1 << 20
    pmax = 1 << 20
    for step in range(3):
        pos, index, weight = s.draw(128)
        want = P.draw(table, 128, 12, step, True, 0.4, subset)
        assert torch.equal(pos.cpu(), torch.from_numpy(want[0]))
        assert torch.equal(index.cpu(), torch.from_numpy(want[1]))
        np.testing.assert_allclose(weight.cpu().numpy(), want[2], rtol=1e-6)
        loss = torch.rand(128, generator=torch.Generator().manual_seed(step)) * 4
        s.update(pos, loss.cuda())
        table, pmax = P.update(table, want[0], loss.numpy(), base, 0.5, 1e-3, pmax)
        assert (s.table() == table).all() and s.running_max() == pmax
    assert s.counter == 3
    np.testing.assert_allclose(s.priorities().numpy(), table / 2.0 ** 20, rtol=0)
    # a second sampler restored from the first draws what the first draws next
    t = PrioritySampler(n, "cuda", base=base, subset=subset, n_frames=4000, alpha=0.5, beta=0.4,
                        seed=12)
    t.load_state_dict(s.state_dict())
    a, b = s.draw(64), t.draw(64)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- end to end ---------------------------------------------------------------------------------------
H, W = 88, 200


@functools.lru_cache(maxsize=None)
def _weights():
    from cilrs_mi355 import CILRS
    return O.portable_state_dict(CILRS(4, 0.0).state_dict(), 0)


def make_trainer(cfg=None, precision="fp32", dropout=0.0):
    from cilrs_mi355 import CILRS, CONFIG_A, Trainer
    m = CILRS(4, dropout=dropout)
    m.load_state_dict(_weights(), strict=True)
    return Trainer(m.cuda(), cfg or CONFIG_A, precision=precision)


@functools.lru_cache(maxsize=None)
def dataset():
    from cilrs_mi355 import data as D
    g = torch.Generator().manual_seed(8)
    n = 64
    cache = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    speed = torch.rand(n, generator=g).cuda()
    command = torch.randint(0, 4, (n,), generator=g).cuda()
    targets = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    return D.DeviceDataset.from_tensors(cache, speed, command, targets)


class Recording:
    """A PrioritizedBatchLoader seen through train_one_epoch: keeps every batch, its positions,
    indices and weights, the row losses handed back and the table before and after each step."""

    def __init__(self, loader):
        self.ld = loader
        self.batches, self.pos, self.index, self.weight = [], [], [], []
        self.rows, self.before, self.after = [], [], []

    @property
    def last_weight(self):
        return self.ld.last_weight

    def feedback(self, rows):
        self.rows.append(rows.clone())
        self.ld.feedback(rows)
        self.after.append(self.ld.sampler.table())

    def __iter__(self):
        it = iter(self.ld)
        while True:
            self.before.append(self.ld.sampler.table())
            try:
                b = next(it)
            except StopIteration:
                self.before.pop()
                return
            self.batches.append(tuple(t.clone() for t in b))
            self.pos.append(self.ld.last_pos.clone())
            self.index.append(self.ld.last_index.clone())
            self.weight.append(self.ld.last_weight.clone())
            yield b


def test_alpha_zero_beta_zero_is_the_plain_step():
    from cilrs_mi355 import CachedBatchLoader, PrioritizedBatchLoader
    from cilrs_mi355.loop import train_one_epoch
    ds = dataset()
    idx = np.arange(5, 29)                                       # 24 frames: three batches of 8
    a, b = make_trainer(), make_trainer()
    rec = Recording(PrioritizedBatchLoader(ds, idx, 8, seed=3, alpha=0.0, beta=0.0))
    assert len(rec.ld) == 3
    out = train_one_epoch(a, rec)
    assert len(rec.batches) == 3 and a.rows_calls == 3 and np.isfinite(out["total"])
    for k, batch in enumerate(rec.batches):
        assert torch.equal(rec.weight[k], torch.ones(8, device="cuda"))
        index = rec.index[k]
        assert torch.equal(index, torch.from_numpy(idx).cuda()[rec.pos[k]])
        assert torch.equal(batch[1], ds.speed[index]) and torch.equal(batch[2], ds.command_dev[index])
        b.train_step(*batch)
    assert b.rows_calls == 0
    assert torch.equal(a.eng.params, b.eng.params)
    assert torch.equal(a.exp_avg_sq, b.exp_avg_sq) and torch.equal(a.eng.bn, b.eng.bn)
    # alpha = 0: the table stays the class-balanced base
    from cilrs_mi355.data import class_balanced_weights
    base = class_balanced_weights(ds.command[idx]).astype(np.float32)
    assert (rec.after[-1] == P.fill(base, 24)).all()
    # a plain loader through the same loop takes the old entry
    train_one_epoch(b, CachedBatchLoader(ds, idx, 8, True, seed=3))
    assert b.rows_calls == 0 and b.step_count == 6
    # eval-mode rows of one batch: the definition on the model's own eval outputs
    batch = rec.batches[0]
    rows = a.row_losses([batch])
    with torch.no_grad():
        pc, ps = a.model(batch[0], batch[1], batch[2])
    want = P.loss_rows(pc.cpu().numpy(), batch[3].cpu().numpy(), ps.cpu().numpy(),
                       batch[1].cpu().numpy(), 0, W4[0])
    np.testing.assert_allclose(rows.cpu().numpy(), want, rtol=2e-7, atol=0)
    assert a.rows_calls == 4


def _three_epochs(trainer, loader, epochs=3):
    from cilrs_mi355.loop import train_one_epoch
    rec = Recording(loader)
    for _ in range(epochs):
        train_one_epoch(trainer, rec)
    return rec


def test_prioritised_epochs_follow_the_definition_and_resume():
    from cilrs_mi355 import PrioritizedBatchLoader
    from cilrs_mi355.data import class_balanced_weights
    ds = dataset()
    idx = np.arange(40, 55)                                      # 15 frames: one batch of 8 an epoch
    kw = dict(seed=9, alpha=0.6, beta=0.4)
    tr = make_trainer()
    rec = _three_epochs(tr, PrioritizedBatchLoader(ds, idx, 8, **kw))
    assert len(rec.batches) == 3 and tr.rows_calls == 3
    base = class_balanced_weights(ds.command[idx]).astype(np.float32)
    sampler = rec.ld.sampler
    assert (rec.before[0] == P.fill(base, 15)).all()
    pmax = 1 << 20
    for k in range(3):
        # the draw: the definition on the device's own table, exactly
        want = P.draw(rec.before[k], 8, sampler.seed, k, True, 0.4, idx)
        assert torch.equal(rec.pos[k].cpu(), torch.from_numpy(want[0])), k
        assert torch.equal(rec.index[k].cpu(), torch.from_numpy(want[1])), k
        np.testing.assert_allclose(rec.weight[k].cpu().numpy(), want[2], rtol=1e-6)
        # the update: the definition on the read-back row losses and positions
        table, pmax = P.update(rec.before[k], want[0], rec.rows[k].cpu().numpy(), base, 0.6, 1e-3,
                               pmax)
        diff = np.abs(rec.after[k].astype(np.int64) - table.astype(np.int64))
        assert (diff <= np.maximum(1, table.astype(np.float64) * 2.0 ** -20)).all(), k
        assert (rec.rows[k] > 0).all() and torch.isfinite(rec.rows[k]).all()
        if k < 2:
            assert (rec.after[k] == rec.before[k + 1]).all()
    assert (rec.after[2] != rec.before[0]).any()
    # restored after the first epoch: a fresh trainer repeats it, a fresh loader takes the state
    tr2 = make_trainer()
    first = _three_epochs(tr2, PrioritizedBatchLoader(ds, idx, 8, **kw), epochs=1)
    assert torch.equal(first.pos[0], rec.pos[0])
    state = first.ld.state_dict()
    resumed = PrioritizedBatchLoader(ds, idx, 8, **kw)
    resumed.load_state_dict(state)
    rest = _three_epochs(tr2, resumed, epochs=2)
    for k in (1, 2):
        assert torch.equal(rest.index[k - 1], rec.index[k]), k
        assert torch.equal(rest.pos[k - 1], rec.pos[k]), k
        assert torch.equal(rest.batches[k - 1][0], rec.batches[k][0]), k
    assert torch.equal(tr.eng.params, tr2.eng.params)


@pytest.mark.parametrize("case", ["bf16_config_b", "lamb_sam_clip", "finetune_layer1"])
def test_weighted_step_in_the_other_configurations(case):
    """precision, clipping, dropout, LAMB, SAM and a fine-tuning cut take the weights and the rows
    without anything else: the step runs, stays finite, feeds the table, and SAM's second pass is
    weighted too."""
    from cilrs_mi355 import CONFIG_B, PrioritizedBatchLoader, TrainConfig
    from cilrs_mi355.loop import train_one_epoch
    ds = dataset()
    if case == "bf16_config_b":
        tr, passes = make_trainer(CONFIG_B, precision="bf16", dropout=0.5), 1
    elif case == "finetune_layer1":
        tr, passes = make_trainer(), 1
        tr.model.freeze("layer1")
        frozen = tr.eng.params[:tr.eng.trainable_begin(2)].clone()
    else:
        cfg = TrainConfig(name="L", optimizer="lamb", sam_rho=0.05, grad_clip=1.0, loss="l1",
                          loss_weights=(5.0, 1.0, 1.0, 0.5))
        tr, passes = make_trainer(cfg), 2
    rec = Recording(PrioritizedBatchLoader(ds, np.arange(30, 46), 8, seed=1))     # two batches
    out = train_one_epoch(tr, rec)
    assert len(rec.batches) == 2 and tr.rows_calls == 2 * passes and tr.step_count == 2
    assert all(np.isfinite(v) for v in out.values())
    assert (rec.after[1] != rec.before[0]).any() and all((r > 0).all() for r in rec.rows)
    assert all(float(w.max()) == 1.0 and float(w.min()) > 0 for w in rec.weight)
    if case == "finetune_layer1":
        assert tr.group_lag[:2] == [2, 2] and torch.equal(tr.eng.params[:frozen.numel()], frozen)


def test_data_parallel_routes_take_the_weights(tmp_path):
    """world size 1, both routes: the weighted step with row losses is bit for bit the single-GPU
    one (each rank keeps its own table: no collective beyond the gradient buckets)."""
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer, CILRS
    ds = dataset()
    g = torch.Generator().manual_seed(5)
    index = torch.randint(0, 64, (8,), generator=g).numpy()
    from cilrs_mi355 import data as D
    batch = ds.assemble(index, D.identity_params(8))
    weight = (torch.rand(8, generator=g) * 0.9 + 0.1).cuda()

    def run(tr):
        rows = torch.full((8,), float("nan"), device="cuda")
        for _ in range(2):
            tr.train_step(*batch, sample_weight=weight, row_loss=rows)
        torch.cuda.synchronize()
        return tr.eng.params.clone(), rows.clone(), tr.loss_buf[:6].clone()

    want = run(make_trainer())
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for bucket in (True, False):
            m = CILRS(4, dropout=0.0)
            m.load_state_dict(_weights(), strict=True)
            tr = Trainer(m.cuda(), CONFIG_A, process_group=dist.group.WORLD)
            tr.bucket_optimizer = bucket
            got = run(tr)
            assert tr.rows_calls == 2 and tr.reducer.collectives == 6
            assert all(torch.equal(a, b) for a, b in zip(got, want)), bucket
    finally:
        dist.destroy_process_group()
    assert torch.isfinite(want[1]).all() and (want[1] > 0).all()
